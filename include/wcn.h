/*
 * wcn.h - C-ABI of the MI355X (gfx950) sparse-3D-convolution engine.
 *
 * This is the drop-in boundary for the SparseConv3d hot path: every entry point replaces one
 * binding of the reference's pybind11 module `warpconvnet._C` (the file:line cited at each
 * declaration is relative to the reference tree).  Conventions:
 *
 *   - plain C: raw device pointers, sizes, and a `hipStream_t` passed as `void*`; no torch types;
 *   - the CALLER allocates every buffer (outputs, workspaces); the library never allocates or frees
 *     device memory; its only process-wide state is a per-device once-flag (kernel attributes), so the
 *     entry points are re-entrant.  A single call is a fixed sequence of launches on the stream and may be
 *     stream-captured; a kernel-map BUILD as the host drives it is not a capturable unit - the host reads
 *     the status word / pair count (pinned mirror written by wcn_kmap_tally_sort) and may rebuild with a
 *     larger block table or the strict insert, exactly as the reference syncs at torch_discrete.py:272;
 *   - every launch goes to the stream argument and is asynchronous; nothing here synchronises;
 *   - return value: 0 on success, negative `wcn_status` otherwise (same numbering as the reference's
 *     `GemmStatus`, warpconvnet/csrc/include/gemm_error_codes.h:7-15);
 *   - data-dependent failures (hash table full, coordinate out of packed range, pair-buffer
 *     overflow) are reported through a device status word the caller reads back when it chooses
 *     (reference: warpconvnet/geometry/coords/search/_packed_base.py:113-120).
 *
 * All index tensors are int32.  Feature tensors are row-major [N, C].
 */
#ifndef WCN_H_
#define WCN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* wcn_stream_t; /* hipStream_t */

/* Status codes: numbering of reference GemmStatus (include/gemm_error_codes.h:7-15). */
enum wcn_status {
  WCN_SUCCESS = 0,
  WCN_ERROR_PROBLEM_NOT_SUPPORTED = -1,
  WCN_ERROR_KERNEL_INITIALIZATION = -2,
  WCN_ERROR_KERNEL_EXECUTION = -3,
  WCN_ERROR_UNSUPPORTED_CONFIG = -4,
  WCN_ERROR_INVALID_PARAMETERS = -5,
  WCN_ERROR_MIXED_INPUT_UNSUPPORTED = -6
};

enum wcn_dtype { WCN_F32 = 0, WCN_F16 = 1, WCN_BF16 = 2 };

/* Bits of the device status word written by the kernel-map kernels. */
enum wcn_kmap_flag {
  WCN_FLAG_TABLE_FULL = 1,      /* hash insert ran out of slots   (reference hash_table.cuh:60-62)   */
  WCN_FLAG_COORD_RANGE = 2,     /* batch not in [0,511] or coord not in [-131072,131071]
                                   (reference packed_hashmap.py:66-82 raises ValueError)            */
  WCN_FLAG_PAIR_OVERFLOW = 4,   /* in_maps/out_maps capacity smaller than the number of pairs       */
  WCN_FLAG_DUPLICATE_COORD = 8, /* informational: the inserted coordinates are not all distinct (the smallest row wins,
                                   so the centre neighbour of a later duplicate is not the row itself)          */
  WCN_FLAG_NEED_STRICT = 16,    /* binned builder, strict = 0: a duplicate coordinate kept a row that is not the smallest
                                   one - the tables are NOT valid, rebuild with strict = 1                         */
  WCN_FLAG_ROW_OVERFLOW = 32    /* binned builder, compact = 1: a row has more than 15 neighbours and does not fit a compact
                                   row - the tables are NOT valid, rebuild with compact = 0                        */
};

/* ---- misc ------------------------------------------------------------------------------------ */
int wcn_abi_version(void);
/* reference: _C.gemm.gemm_status_to_string (bindings/gemm_bindings.cpp) */
const char* wcn_status_string(int status);

/* ---- packed 64-bit coordinate hash table -------------------------------------------------------
 * Key = 1<<63 | batch(9b)<<54 | x(18b)<<36 | y(18b)<<18 | z(18b)   (reference hash_functions.cuh:40-44)
 * Slot = 16 bytes {uint64 key, int32 value, int32 pad}: one 16-B load per probe returns key AND
 * value (the reference keeps two arrays -> two random loads per hit).  Empty key = 0, value = row
 * index of the inserted coordinate; duplicates keep the SMALLEST row index (deterministic; the
 * reference keeps whichever CAS wins, hash_table.cuh:36-63).  Splitmix64 & (capacity-1), linear
 * probing (hash_functions.cuh:75-84, hash_table.cuh:94-108).  capacity must be a power of two.
 */
/* reference: _C.cuhash.packed_prepare (bindings/cuhash_bindings.cpp:244-262, cuhash_hash_table.cu:19-25) */
int wcn_hash_prepare(void* slots, int64_t capacity, wcn_stream_t stream);
/* reference: _C.cuhash.packed_insert (cuhash_hash_table.cu:179-220); coords int32 [n,4]; status int32[1] (OR of wcn_kmap_flag) */
int wcn_hash_insert(void* slots, int64_t capacity, const int32_t* coords, int64_t n, int32_t* status,
                    wcn_stream_t stream);
/* reference: _C.cuhash.packed_search (cuhash_hash_table.cu:222-262); results int32 [m], -1 on miss */
int wcn_hash_search(const void* slots, int64_t capacity, const int32_t* queries, int64_t m,
                    int32_t* results, wcn_stream_t stream);

/* ---- kernel map ----------------------------------------------------------------------------------
 * Neighbour table layout is ROW-major: nbr[m*kp + k] = input row matched by output row m at kernel
 * offset k, or -1 (kp = wcn_kmap_row_pitch(K), rows are 32-B aligned so a tile of rows is one
 * contiguous slab).  The reference's `found_in_coord_index` is the transpose [K, M]
 * (cuhash_kernel_map.cu:93-134); `wcn_kmap_transpose` converts for consumers that want that layout.
 * Kernel offset enumeration: k = (i*ky + j)*kz + l -> offset ((i-cx)*dx, (j-cy)*dy, (l-cz)*dz) with
 * c = (size-1)/2 for odd sizes and 0 for even sizes (torch_discrete.py:24-56, kernel_map.cuh:34-54).
 * Query coordinate = out_coord * stride (torch_discrete.py:352-361).
 */
int32_t wcn_kmap_row_pitch(int32_t num_offsets);
int32_t wcn_kmap_mask_words(int32_t num_offsets);
/* number of 256-row bucket tiles for m query rows, rounded up to a multiple of 4 (rows of the counts array stay 16-B
 * aligned); the counts buffer holds wcn_kmap_counts_bytes(m, K) bytes: K rows of tile counts, K totals, a ticket word */
int64_t wcn_kmap_num_blocks(int64_t m);
size_t wcn_kmap_counts_bytes(int64_t m, int32_t num_offsets);
/* ... and, behind those, the SLAB BOUNDS the scan writes for the weight gradient's team sweep: int32 [17][K] at element
 * wcn_kmap_slab_bounds_offset(m, K) of the counts buffer.  bounds[t][k] = pairs of bucket k whose output row lies in front of
 * row slab t (16 equal slabs of ceil(num_blocks / 16) tiles; bounds[0][k] = 0, bounds[16][k] = the bucket's size).  They
 * describe pair lists in OUTPUT-ROW order inside each bucket - what wcn_kmap_scatter writes from the same counts. */
int64_t wcn_kmap_slab_bounds_offset(int64_t m, int32_t num_offsets);

/* reference: _C.cuhash.packed_kernel_map_size + packed_kernel_map_offset (cuhash_kernel_map.cu:68-134)
 * fused with build_pair_mask (mask_data_kernels.cu:23-44).
 *   query   int32 [m,4]      mask   uint32 [m, mask_words]  (bit k <=> nbr[m][k] >= 0)
 *   nbr     int32 [m,kp]
 */
int wcn_kmap_probe(const void* slots, int64_t capacity, const int32_t* query, int64_t m,
                   const int32_t ksize[3], const int32_t stride[3], const int32_t dilation[3],
                   int32_t* nbr, uint32_t* mask, wcn_stream_t stream);
/* [n, num_dims] int32 coordinates -> [n, num_dims + 1] with the batch index of the row in column 0; `offsets`
 * [num_batches + 1] int32 on the device (may be NULL for one batch).  One launch; replaces the batch-index kernel +
 * torch.cat of warpconvnet/geometry/coords/ops/batch_index.py:90-148. */
int wcn_batch_indexed_coords(const int32_t* coords, int64_t n, int32_t num_dims, const int32_t* offsets,
                             int32_t num_batches, int32_t* out, wcn_stream_t stream);

/* Z-order (Morton) codes of integer coordinates: int64 codes[n].  num_dims 3: rows (x,y,z), 21 bits per axis
 * interleaved with x in the lowest bit of every triple; num_dims 4: rows (b,x,y,z), (b << 48) | interleave of the low 16
 * bits per axis.  `origin` [num_dims] int32 on the DEVICE (may be NULL) is subtracted first (the reference normalises by
 * the per-column minimum); `axis[3]` (host) names the spatial column that feeds the x / y / z slot (MORTON_XYZ = {0,1,2},
 * MORTON_ZYX = {2,1,0}, ...).  Replaces _C.coords.morton_code_20bit / morton_code_16bit
 * (warpconvnet/csrc/morton_code.cu:27-103, call site geometry/coords/ops/serialization.py:196-245). */
int wcn_morton_code(const int32_t* coords, int64_t n, int32_t num_dims, const int32_t* origin, const int32_t axis[3],
                    int64_t* codes, wcn_stream_t stream);

/* LDS-binned neighbour search for SUBMANIFOLD maps (query coords == input coords, stride 1): replaces
 * wcn_hash_insert + wcn_kmap_probe.  The hash table is BLOCK-level: voxels are binned into 8^3 blocks, every occupied
 * block owns a dense 512-cell sub-grid of row ids (one plain 4-B store per voxel), and one wavefront per block stages
 * its sub-grid and the halo of the 26 neighbouring sub-grids in an LDS grid and answers all K probes from LDS.  Same
 * outputs as the hash path (bit-exact), incl. the range flags in *status (the status word is CLEARED by this call).
 *   max_blocks  capacity of the block table (occupied 8^3 blocks); more blocks -> WCN_FLAG_TABLE_FULL, tables invalid,
 *               the caller retries with max_blocks = n (always enough) - workspace = wcn_kmap_binned_workspace(n, max_blocks)
 *   strict      0: cells are written with plain stores; rows of duplicate coordinates are repaired by
 *               wcn_kmap_tally_sort, which raises WCN_FLAG_NEED_STRICT when a cell did not keep the smallest row
 *               (the caller then rebuilds with strict = 1: atomicMin, ~2.5x the store cost)
 *   mask        rows that no block has enumerated yet (duplicates) carry 0x80000000 in their LAST mask word until
 *               wcn_kmap_tally_sort repairs them, which is why K % 32 == 0 is not supported here
 * Returns WCN_ERROR_PROBLEM_NOT_SUPPORTED when the kernel halo (max |offset| per axis, dilation included) exceeds 8 cells or K % 32 == 0
 * (wcn_kmap_binned_supported == 0): the caller then uses the hash path.
 *   compact     0: nbr is the dense [n, kp] table above.  1 (wcn_kmap_compact_supported: one mask word and 17 <= K <= 31, e.g. the
 *               3 x 3 x 3 kernel): nbr is [n, 16] COMPACT rows - word 0 = the row's mask, words 1 .. popcount(mask) = the neighbour
 *               rows of its SET offsets in ascending k, the rest unspecified - 64 B per row instead of 128 for 4 - 9 neighbours
 *               (round 6: half the bytes for the builder's stores, the pair scatter and both gather GEMMs).  A row with more
 *               than 15 neighbours raises WCN_FLAG_ROW_OVERFLOW (tables invalid, rebuild with compact = 0).  Consumers of compact
 *               tables: wcn_kmap_tally_sort / wcn_kmap_scatter (compact = 1), the gather GEMMs where
 *               wcn_conv_compact_table_supported (`mask` = NULL), wcn_kmap_densify for everything else.
 * reference being replaced: cuhash_hash_table.cu:179-220 + cuhash_kernel_map.cu:93-134. */
size_t wcn_kmap_binned_workspace(int64_t n, int64_t max_blocks);
int wcn_kmap_binned_supported(const int32_t ksize[3], const int32_t dilation[3]);
int wcn_kmap_compact_supported(int32_t num_offsets);
int wcn_kmap_build_binned(const int32_t* coords, int64_t n, const int32_t ksize[3], const int32_t dilation[3],
                          int64_t max_blocks, int32_t strict, int32_t compact, void* workspace, size_t workspace_bytes,
                          int32_t* nbr, uint32_t* mask, int32_t* status, wcn_stream_t stream);
/* compact rows [m, 16] -> the dense table nbr [m, kp] (-1 = absent): for consumers without a compact path. */
int wcn_kmap_densify(const int32_t* nbr_compact, int64_t m, int32_t num_offsets, int32_t* nbr, wcn_stream_t stream);
/* Everything between the neighbour table and the ONE host read of a build:
 *   tally  per-(offset, tile) pair counts from the masks, the first digit histogram of the mask sort, and - when
 *          `binned_workspace` (the workspace of the wcn_kmap_build_binned call that produced nbr / mask, with its n and
 *          max_blocks) is given - repair of the rows of duplicate coordinates
 *   scan   offsets int32 [K+1] on the device and, if `host_mirror` (K + 3 int32 of pinned, device-accessible HOST
 *          memory) is given, offsets ++ [*status] ++ [ready] there in the same launch: `ready` (cleared by the caller)
 *          becomes 1 last, behind a system-scope fence, so the host may spin on it instead of waiting for an event
 *   sort   perm = rows by descending mask (wcn_mask_argsort), the first digit already counted
 *   pairs  (in_maps / out_maps given, pair_capacity > 0: round 6) the pair lists of wcn_kmap_scatter queued behind the sort by
 *          the same call, at a capacity the caller guesses before the pair count is known.  A capacity below the pair count:
 *          nothing past it is written, the caller compares it with offsets[K] (in the mirror by then) and runs
 *          wcn_kmap_scatter at the exact length.
 *   compact  nbr holds COMPACT rows (wcn_kmap_build_binned)
 * counts: wcn_kmap_counts_bytes(m, K) bytes, consumed by wcn_kmap_scatter.  sort_workspace:
 * wcn_kmap_tally_sort_workspace(m) bytes.  reference: postprocess_count + torch.cumsum + mask_argsort
 * (cuhash_kernel_map.cu:508-544, torch_discrete.py:268-272, mask_data_kernels.cu:187-220). */
size_t wcn_kmap_tally_sort_workspace(int64_t m);
int wcn_kmap_tally_sort(uint32_t* mask, int32_t* nbr, int64_t m, int32_t num_offsets, int32_t* counts, int32_t* offsets,
                        int32_t* status, int32_t* host_mirror, int32_t* perm, void* sort_workspace,
                        size_t sort_workspace_bytes, const int32_t* coords, void* binned_workspace, int64_t binned_n,
                        int64_t max_blocks, int32_t compact, int32_t* in_maps, int32_t* out_maps, int64_t pair_capacity,
                        wcn_stream_t stream);
/* counts[k][b] = pairs of offset k in the 256-row tile b (k-major, from the masks); counts = wcn_kmap_counts_bytes bytes.
 * reference: _C.cuhash.postprocess_count (cuhash_kernel_map.cu:508-544). */
int wcn_kmap_count(const uint32_t* mask, int64_t m, int32_t num_offsets, int32_t* counts, wcn_stream_t stream);
/* exclusive scan of counts over tiles (in place, one workgroup per offset) and over offsets ->
 * offsets int32 [K+1].  `counts` as left by wcn_kmap_count (the tail receives the bucket totals).
 * reference: host torch.cumsum in torch_discrete.py:268-272. */
int wcn_kmap_scan(int32_t* counts, int64_t num_blocks, int32_t num_offsets, int32_t* offsets,
                  wcn_stream_t stream);
/* the same, and in the same launch offsets[0..K] ++ [*status] ++ [ready = 1] are also written to `host_mirror` - K + 3 int32 of pinned
 * (device-accessible) HOST memory: the one host read of a build (torch_discrete.py:268-272 does `.item()` per value)
 * becomes an event wait behind this kernel, no copy command. */
int wcn_kmap_scan_to_host(int32_t* counts, int64_t num_blocks, int32_t num_offsets, int32_t* offsets, const int32_t* status,
                          int32_t* host_mirror, wcn_stream_t stream);
/* deterministic compaction (pairs of one offset ordered by output row).
 * reference: _C.cuhash.postprocess_scatter (cuhash_kernel_map.cu:546-599, order there is racy).
 * pair_capacity = length of in_maps/out_maps; sets WCN_FLAG_PAIR_OVERFLOW in *status if too small. */
int wcn_kmap_scatter(const int32_t* nbr, const uint32_t* mask, int64_t m, int32_t num_offsets,
                     const int32_t* counts, const int32_t* offsets, int32_t* in_maps, int32_t* out_maps, int64_t pair_capacity,
                     int32_t* status, int32_t compact, wcn_stream_t stream);
/* ---- strided layers from the cell table of the FINE set (no global hash table) ------------------------------------------
 * `cells_workspace` = the workspace of a wcn_kmap_build_binned call on the fine coordinates (with its n and max_blocks)
 * whose status word came back without TABLE_FULL / NEED_STRICT.
 * Down-sampling (reference coords/ops/stride.py:18-56: floor-divide, hash de-duplicate, unique): strides 1 / 2 / 4 / 8 per
 * axis, so that a coarse cell lies inside one 8^3 block (wcn_cells_stride_supported).
 *   _count  flags = one bit per fine row: "first (smallest) row of its coarse cell" (uint64 per 64 rows); counts
 *           [wcn_cells_stride_tiles(n) + 1] int32 = survivors in front of every 256-row tile, the last entry their total;
 *           out_offsets[b] = survivors with a batch index < b, b = 0 .. num_batches (the batch offsets of the output; the
 *           rows must be sorted by batch index, as everywhere)
 *   _emit   out_coords [M, 4] = (b, x >> log2 sx, ...) of the survivors in input order; first_rows [M] (may be NULL) their
 *           fine rows; nbr [M, kp] / mask [M] (both or neither): the kernel map of a convolution with kernel_size == stride,
 *           dilation 1 - nbr[m][(i*sy + j)*sz + l] = fine row in cell (x0 + i, y0 + j, z0 + l) of the coarse cell, or -1
 * wcn_kmap_probe_cells: wcn_kmap_probe answered from the cell table - same table / mask layout, same 18-bit wrap, the
 * smallest row of a duplicated coordinate - for any kernel size, stride and dilation; replaces wcn_hash_insert +
 * wcn_kmap_probe when the input set already has a cell table.  reference: cuhash_kernel_map.cu:93-134;
 * coarse-to-fine search geometry/coords/search/hierarchical_search.py:25-66. */
/* the cell table alone (prepare + inserts + finish of wcn_kmap_build_binned, strict insert: the smallest row of a duplicated
 * coordinate wins by construction) for a coordinate set that has no submanifold build yet - e.g. a network whose first
 * spatial layer is strided.  `scratch`: n uint32.  status: WCN_FLAG_TABLE_FULL (retry with a larger max_blocks) /
 * WCN_FLAG_COORD_RANGE.  workspace: wcn_kmap_binned_workspace(n, max_blocks). */
int wcn_kmap_cells_build(const int32_t* coords, int64_t n, int64_t max_blocks, void* workspace, size_t workspace_bytes,
                         uint32_t* scratch, int32_t* status, wcn_stream_t stream);
int wcn_cells_stride_supported(const int32_t stride[3]);
int64_t wcn_cells_stride_tiles(int64_t n);
int wcn_cells_stride_count(const void* cells_workspace, int64_t n, int64_t max_blocks, const int32_t* coords,
                           const int32_t stride[3], uint64_t* flags, int32_t* counts, int32_t num_batches,
                           int32_t* out_offsets, wcn_stream_t stream);
int wcn_cells_stride_emit(const void* cells_workspace, int64_t n, int64_t max_blocks, const int32_t* coords,
                          const int32_t stride[3], const uint64_t* flags, const int32_t* counts, int32_t* out_coords,
                          int32_t* first_rows, int32_t* nbr, uint32_t* mask, wcn_stream_t stream);
int wcn_kmap_probe_cells(const void* cells_workspace, int64_t n_in, int64_t max_blocks, const int32_t* query, int64_t m,
                         const int32_t ksize[3], const int32_t stride[3], const int32_t dilation[3], int32_t* nbr,
                         uint32_t* mask, wcn_stream_t stream);
/* nbr [m,kp] -> pair_table [K,m]   (the reference layout, cuhash_kernel_map.cu:133) */
int wcn_kmap_transpose(const int32_t* nbr, int64_t m, int32_t num_offsets, int32_t* pair_table,
                       wcn_stream_t stream);
/* reverse table for dgrad of strided / transposed maps: rev_nbr[in][k] = out, rev_mask bit k.
 * The call itself pre-fills rev_nbr with -1 and rev_mask with 0.  `max_pairs` bounds the launch
 * (length of in_maps/out_maps); the true pair count is read from offsets[K] on the device.
 * reference: _C.gemm.build_reverse_mask_data_cuda (mask_data_kernels.cu:101-124). */
int wcn_kmap_reverse(const int32_t* in_maps, const int32_t* out_maps, const int32_t* offsets,
                     int32_t num_offsets, int64_t max_pairs, int64_t n_in, int32_t* rev_nbr,
                     uint32_t* rev_mask, wcn_stream_t stream);
/* reference: _C.gemm.csr_to_pair_table_cuda + build_pair_mask_cuda (mask_data_kernels.cu:23-82):
 * rebuild nbr/mask from a CSR map (used for maps that were swapped for transposed conv). */
int wcn_kmap_from_csr(const int32_t* in_maps, const int32_t* out_maps, const int32_t* offsets,
                      int32_t num_offsets, int64_t max_pairs, int64_t n_out, int32_t* nbr, uint32_t* mask,
                      wcn_stream_t stream);
/* permutation of rows sorted by descending mask word 0 (rows with equal neighbourhood pattern become
 * adjacent so a wavefront can skip absent offsets).  reference: _C.gemm.mask_argsort_cuda
 * (mask_data_kernels.cu:187-220, CUB radix sort).  Hand-written stable LSD radix sort (ties keep ascending
 * row order); `num_bits` = number of significant low bits of word 0 (min(K, 32)) bounds the passes.
 * workspace: wcn_mask_argsort_workspace(n) bytes. */
size_t wcn_mask_argsort_workspace(int64_t n);
int wcn_mask_argsort(const uint32_t* mask, int32_t mask_words, int32_t num_bits, int64_t n, int32_t* perm,
                     void* workspace, size_t workspace_bytes, wcn_stream_t stream);
/* The row order the gather GEMMs cut into tiles (and the `perm` wcn_kmap_tally_sort writes): a tile runs one step per offset ANY of
 * its rows has, so rows are grouped to keep the UNION of a tile's masks small.  Odd kernel volumes K = 2c + 1 <= 31: stable sort
 * by a key of the same width as the mask - mirror-image offsets (k, K-1-k) paired, "which pairs" in the high half, "which member"
 * in the low half, ranked in reflected-Gray order (csrc/mask_sort.h) - 8.8 -> 7.2 steps per 128-row tile on the uniform 1 M scene,
 * unchanged on surface-like scenes.  Any other volume: wcn_mask_argsort.  The GEMM results do not depend on the order.
 * Role of the reference's mask_argsort inside its mask-GEMM path (mask_gemm.py:127-254).  workspace: wcn_mask_argsort_workspace. */
int wcn_mask_tile_order(const uint32_t* mask, int32_t mask_words, int32_t num_offsets, int64_t n, int32_t* perm,
                        void* workspace, size_t workspace_bytes, wcn_stream_t stream);

/* ---- sparse convolution GEMMs ------------------------------------------------------------------
 * Forward  (AB gather-scatter):  y[m]  = sum_k x[nbr[m][k]] . w[k]            w: [K, Cin, Cout]
 * Dgrad    (ABt gather-scatter): dx[n] = sum_k dy[rnbr[n][k]] . w[k]^T
 * Wgrad    (AtB gather-gather):  dw[k] = sum_p x[in_maps[p]]^T . dy[out_maps[p]],  p in bucket k
 * reference semantics: nn/functional/sparse_conv/detail/explicit.py:22-101; fused production kernels
 * _C.mask_gemm.fwd/.dgrad/.wgrad (bindings/mask_gemm_bindings.cu:2071-2123).
 *
 * `algo`: 1 = hip_ref (any channel count / dtype), 2 = hip_mfma (bf16/f16; forward/dgrad: Cin%16==0,
 * Cout in {32,64,96,128,192,256}, K<=32; wgrad: Cin%32==0, Cout%32==0; WCN_ERROR_UNSUPPORTED_CONFIG
 * otherwise).  0 (auto) is resolved by the caller with wcn_mfma_*_supported because the two algorithms
 * take different weight images.  Accumulation is always fp32.
 */
enum wcn_algo { WCN_ALGO_AUTO = 0, WCN_ALGO_REF = 1, WCN_ALGO_MFMA = 2 };

/* 1 if the MFMA kernels cover the shape (so the caller can resolve "auto" without a trial launch). */
int wcn_mfma_gather_supported(int32_t cin, int32_t cout, int32_t num_offsets, int32_t dtype);
int wcn_mfma_wgrad_supported(int32_t cin, int32_t cout, int32_t dtype);
/* 1 x 1 x 1 convolutions (reference shortcut helper.py:206-213: feats @ weight[0]): wcn_conv_gather_gemm with num_offsets = 1
 * and nbr = mask = perm = NULL treats every row as its own only neighbour - the dense [N, cin] x [cin, cout] product streamed
 * through the gather kernel at its HBM rate (the vendor GEMM runs these skinny shapes at 0.15-0.33 of it,
 * profiles/r04_unet_1M_roofline.md).  Shapes: cin % 32 == 0, cin >= 64, cout in {64, 96, 128}, f16 / bf16. */
int wcn_conv_identity_supported(int32_t cin, int32_t cout, int32_t dtype);
/* The NARROW 1 x 1 x 1 layers (same reference line, helper.py:206-213): y[n, cout] = x[n, cin] * W (+ bias) for any
 * cin <= 128, cout <= 96 - the 3 -> 32 stem and the 96 -> 20 head of a MinkUNet and their input gradients - as one streaming
 * kernel (csrc/dense_rows.hip; the vendor GEMM serves a 20- or 3-column operand at 0.09-0.15 of the HBM rate).  `w` is the
 * layer's matrix as stored, row-major: [cin, cout], or [cout, cin] with w_transposed = 1 (the input gradient dy * W^T reads the
 * forward weight in place); its elements are fp32 (w_is_f32 = 1, master weights) or `dtype`, converted in the kernel - no
 * packed image.  The rows `x` are `dtype`, or fp32 with x_is_f32 = 1 (rounded to `dtype` on the fly, as a cast in front of the
 * product would).  `y`: [n, cout] in `dtype` (f16 / bf16), fp32 accumulation, optional fp32 bias[cout]. */
int wcn_dense_rows_supported(int32_t cin, int32_t cout, int32_t dtype);
int wcn_dense_rows(const void* x, int32_t x_is_f32, const void* w, int32_t w_is_f32, int32_t w_transposed, const float* bias,
                   void* y, int64_t n, int32_t cin, int32_t cout, int32_t dtype, wcn_stream_t stream);

/* Packed weight image consumed by the MFMA kernels (fragment order, zero padding).  `transpose`=1
 * packs w[k]^T (dgrad); `flip`=1 additionally reverses k (dgrad of a submanifold map reuses the
 * forward table: rnbr[n][k] == nbr[n][K-1-k]).  Returns bytes needed / fills `packed`.  `cin` / `cout` are the kernel-side
 * roles (reduce over cin, produce cout); the image holds num_offsets * round_up(cin, 64) * cout elements (the channel-split
 * kernels reduce in 64-channel chunks and zero-pad a trailing 32-channel chunk) - size `packed` with wcn_packed_weight_bytes;
 * `packed_bytes` = the size of the caller's buffer: WCN_ERROR_INVALID_PARAMETERS (nothing launched) if it is smaller than that. */
size_t wcn_packed_weight_bytes(int32_t num_offsets, int32_t cin, int32_t cout, int32_t dtype, int32_t transpose);
int wcn_pack_weight(const void* w, int32_t num_offsets, int32_t cin, int32_t cout, int32_t dtype,
                    int32_t transpose, int32_t flip, void* packed, size_t packed_bytes, wcn_stream_t stream);
/* the same packed image (`dtype` = WCN_F16 / WCN_BF16) straight from fp32 master weights, rounded to nearest even like the
 * framework's cast: one launch instead of cast + pack per convolution and direction. */
int wcn_pack_weight_f32(const float* w, int32_t num_offsets, int32_t cin, int32_t cout, int32_t dtype, int32_t transpose,
                        int32_t flip, void* packed, size_t packed_bytes, wcn_stream_t stream);
/* Both images a training step needs - forward (w [K, cin, cout] as is) and dgrad (kernel-side roles exchanged: transposed, and
 * k-flipped when `flip_dgrad`, i.e. for a submanifold map whose dgrad reads the forward table) - of an fp32 master weight in ONE
 * launch: an optimizer step invalidates both at once.  Shapes: wcn_pack_weight_pair_supported (both directions on the
 * channel-split kernels); sizes: wcn_packed_weight_bytes(K, cin, cout, dtype, 0) and (K, cout, cin, dtype, 1). */
int wcn_pack_weight_pair_supported(int32_t num_offsets, int32_t cin, int32_t cout, int32_t dtype);
int wcn_pack_weight_f32_pair(const float* w, int32_t num_offsets, int32_t cin, int32_t cout, int32_t dtype, int32_t flip_dgrad,
                             void* packed_fwd, size_t packed_fwd_bytes, void* packed_dgrad, size_t packed_dgrad_bytes,
                             wcn_stream_t stream);

/* y = gather-GEMM over a neighbour table.  Serves forward (x, packed w) and dgrad (dy, packed w^T).
 *   in   [n_in, cin]   out [n_out, cout]   nbr [n_out, kp]   mask [n_out, mw]   perm [n_out] or NULL
 *   bias fp32 [cout] or NULL: fused epilogue out += bias (reference adds it afterwards, helper.py:339-342)
 *   w:   for WCN_ALGO_REF the plain [K, cin, cout] tensor (or [K, cout', cin'] with w_transposed=1),
 *        for WCN_ALGO_MFMA the image made by wcn_pack_weight.
 * reference: _C.mask_gemm.fwd / .dgrad (mask_gemm_bindings.cu:2074-2101). */
/* Compact tables (round 6; round 5 carried the mask in column 31 of a dense row instead).  Where wcn_conv_compact_table_supported
 * (channel-split kernel shapes, wcn_kmap_compact_supported(K)), wcn_conv_gather_gemm / _fused / _f32out / wcn_conv_bn_backward accept
 * `mask` = NULL with `nbr` = the COMPACT table of wcn_kmap_build_binned(compact = 1): the rows are expanded into the kernel's index
 * slab - half the table bytes, and no gather of mask[perm[i]] (one 128-B line per row: 128 MB of fabric requests per launch at 1 M
 * rows for 4 MB of masks).  Dense tables (every other builder) always come with their mask. */
int wcn_conv_compact_table_supported(int32_t cin, int32_t cout, int32_t num_offsets, int32_t dtype);
int wcn_conv_gather_gemm(const void* in, const void* w, void* out, const int32_t* nbr,
                         const uint32_t* mask, const int32_t* perm, const float* bias, int64_t n_in,
                         int64_t n_out, int32_t cin, int32_t cout, int32_t num_offsets, int32_t dtype,
                         int32_t algo, int32_t w_transposed, int32_t k_flip, wcn_stream_t stream);

/* Channel groups in ONE launch (weight [K, G, Cin/G, Cout/G]; reference: group index on grid.z of the fused kernel,
 * MaskGemm_forward_64x64x32_1s_flat.h:117-123; sparse_conv.py:147-157).  Per-group widths cin_g x cout_g must be a shape
 * of the 32x32x16 kernels (wcn_mfma_grouped_supported); feature rows hold all groups side by side ([N, G*cin_g] in,
 * [N, G*cout_g] out), `bias` (optional) has G*cout_g entries.  wcn_pack_weight_grouped writes the G fragment-ordered
 * images back to back in one launch from the forward weight ([K, G, cin_g, cout_g], fp32 or the storage dtype);
 * transpose = 1, flip = 1 with swapped widths gives the dgrad images of a submanifold map, as for wcn_pack_weight. */
int wcn_mfma_grouped_supported(int32_t cin_g, int32_t cout_g, int32_t num_offsets, int32_t dtype);
int wcn_pack_weight_grouped(const void* w, int32_t w_is_f32, int32_t num_offsets, int32_t groups, int32_t cin_g,
                            int32_t cout_g, int32_t dtype, int32_t transpose, int32_t flip, void* packed, wcn_stream_t stream);
int wcn_conv_gather_gemm_grouped(const void* in, const void* w_packed, void* out, const int32_t* nbr, const uint32_t* mask,
                                 const int32_t* perm, const float* bias, int64_t n_in, int64_t n_out, int32_t cin_g,
                                 int32_t cout_g, int32_t groups, int32_t num_offsets, int32_t dtype, wcn_stream_t stream);
/* As wcn_conv_gather_gemm with algo = WCN_ALGO_MFMA, but the result is written as fp32 straight from the fp32
 * accumulators (in / w_packed are WCN_F16 or WCN_BF16).  Used for fp32 feature tensors: operands are cast to fp16 with
 * an exact power-of-two rescale by the caller, the product is scaled back in fp32 - the reference's production
 * treatment of fp32 inputs (warpconvnet/nn/functional/sparse_conv/detail/mask_gemm.py:72-103, 696-745). */
int wcn_conv_gather_gemm_f32out(const void* in, const void* w_packed, float* out, const int32_t* nbr,
                                const uint32_t* mask, const int32_t* perm, const float* bias, int64_t n_in,
                                int64_t n_out, int32_t cin, int32_t cout, int32_t num_offsets, int32_t dtype,
                                wcn_stream_t stream);

/* Gather GEMM with the elementwise chain of a ConvBlock folded into the store (the reference runs
 * conv -> BatchNorm1d -> ReLU (+ residual add) as separate kernels, models/mink_unet.py:31-53, 161-175):
 *   out[m][co] = act( (sum_k in[nbr[m][k]] . W[k] + bias[co]) * scale[co] + shift[co] + residual[m][co] )
 * evaluated in fp32 before the single rounding to the storage dtype.  bias / scale+shift / residual may be NULL
 * (scale and shift only together); BatchNorm in inference mode is scale = gamma / sqrt(var + eps),
 * shift = beta - mean * scale; relu != 0 applies max(., 0).  `residual` [n_out, cout] has the storage dtype and must not
 * alias `out`.  MFMA path only (f16 / bf16, shapes of wcn_mfma_gather_supported, `w_packed` from wcn_pack_weight). */
int wcn_conv_gather_gemm_fused(const void* in, const void* w_packed, void* out, const int32_t* nbr, const uint32_t* mask,
                               const int32_t* perm, const float* bias, const float* scale, const float* shift,
                               const void* residual, int32_t relu, int64_t n_in, int64_t n_out, int32_t cin, int32_t cout,
                               int32_t num_offsets, int32_t dtype, wcn_stream_t stream);

/* out[c] = sum_r in[r][c] in fp32 (bias gradient; reference: autograd of `out + bias`, helper.py:339-342).
 * Deterministic two-pass reduction; workspace: wcn_colsum_workspace(channels) bytes. */
size_t wcn_colsum_workspace(int32_t channels);
int wcn_colsum(const void* in, int64_t n, int32_t channels, int32_t dtype, float* out, void* workspace,
               size_t workspace_bytes, wcn_stream_t stream);

/* dw [K, cin, cout] fp32 (overwritten).  workspace: wcn_conv_wgrad_workspace(...) bytes.
 * reference: _C.mask_gemm.wgrad (mask_gemm_bindings.cu:2103-2116), fp32 output. */
size_t wcn_conv_wgrad_workspace(int32_t num_offsets, int32_t cin, int32_t cout, int32_t algo);
int wcn_conv_wgrad(const void* x, const void* dy, float* dw, const int32_t* in_maps,
                   const int32_t* out_maps, const int32_t* offsets, int64_t n_in, int64_t n_out,
                   int32_t cin, int32_t cout, int32_t num_offsets, int32_t dtype, int32_t algo,
                   void* workspace, size_t workspace_bytes, wcn_stream_t stream);

/* Weight gradient + bias gradient in one pass.  As wcn_conv_wgrad with algo = WCN_ALGO_MFMA, and additionally
 * bias_grad[co] = sum over rows r of dy[r][co] (fp32 [cout], overwritten): while the kernel streams bucket
 * `self_offset` - the offset whose pairs are (r, r) for every row r, i.e. the centre of an odd submanifold kernel
 * built from distinct coordinates (WCN_FLAG_DUPLICATE_COORD clear) - it also multiplies a ones-row fragment with the
 * dy fragments it holds, so the column sums come out of the matrix cores with no extra read of dy.  Deterministic.
 * Replaces the autograd reduce of `out + bias` (warpconvnet/nn/functional/sparse_conv/helper.py:339-342).
 * WCN_ERROR_UNSUPPORTED_CONFIG unless wcn_mfma_wgrad_bias_supported (then use wcn_conv_wgrad + wcn_colsum).
 * workspace: wcn_conv_wgrad_workspace(num_offsets, cin, cout, WCN_ALGO_MFMA) bytes. */
int wcn_mfma_wgrad_bias_supported(int32_t cin, int32_t cout, int32_t dtype);
int wcn_conv_wgrad_bias(const void* x, const void* dy, float* dw, const int32_t* in_maps, const int32_t* out_maps,
                        const int32_t* offsets, int64_t n_in, int64_t n_out, int32_t cin, int32_t cout,
                        int32_t num_offsets, int32_t dtype, int32_t self_offset, float* bias_grad, void* workspace,
                        size_t workspace_bytes, wcn_stream_t stream);

/* The MFMA weight gradient (wcn_conv_wgrad, algo = WCN_ALGO_MFMA; with `bias_grad` non-NULL: wcn_conv_wgrad_bias) of a map
 * whose pair lists come with SLAB BOUNDS (wcn_kmap_slab_bounds_offset; device pointer, NULL = none).  Where the rule of
 * csrc/wgrad_plan.h holds - K = 27, one (cin, cout) tile, >= 512 x 512 pairs, the largest off-centre bucket <= 1.10 x their
 * mean, no (slab, offset) range longer than the level the centre pieces fill every workgroup up to - the device sweeps the lists in row-slab TEAMS (the 26 off-centre offsets of a slab side by side on one XCD, so that
 * the repeated gathers of a dY row meet in L2) instead of 512 equal ranges; the decision is made on the device from
 * offsets[] and the bounds, every other launch runs exactly as without them.  Deterministic either way; the two sweeps add
 * the fp32 partial tiles in different orders.  WARPCONVNET_AMD_WGRAD_TEAMS = 0 | auto (default) | force (the size and
 * balance conditions dropped; tests, A/B runs), read per call.  workspace: wcn_conv_wgrad_workspace(..., WCN_ALGO_MFMA).
 * wcn_wgrad_plan_host (host only, host pointers): the segments {bucket, begin, end} x (1 or 2) workgroup g of `grid`
 * sweeps under the team plan; 0 = the rule refuses; `mode` 0 / 1 / 2 = off / auto / force. */
int wcn_conv_wgrad_teams(const void* x, const void* dy, float* dw, const int32_t* in_maps, const int32_t* out_maps,
                         const int32_t* offsets, const int32_t* slab_bounds, int64_t n_in, int64_t n_out, int32_t cin,
                         int32_t cout, int32_t num_offsets, int32_t dtype, int32_t self_offset, float* bias_grad,
                         void* workspace, size_t workspace_bytes, wcn_stream_t stream);
int wcn_wgrad_plan_host(const int32_t* offsets, const int32_t* slab_bounds, int32_t num_offsets, int32_t grid, int32_t tiles,
                        int32_t mode, int32_t g, int64_t* out);

/* ---- depthwise sparse convolution (weight [K, C], same dtype as the features) ----------------------------------------
 * reference semantics: warpconvnet/nn/functional/sparse_conv_depth.py:227-306 (explicit depthwise forward/backward);
 * replaces _C.fma.implicit_fma / _C.fma.implicit_reduction (call sites sparse_conv_depth.py:309-421).
 *
 * wcn_dwconv_gather: out[r][c] = bias[c] + sum_k in[nbr[r][kt]][c] * w[kw][c], kt = k_flip ? K-1-kw : kw, fp32
 *   accumulate, fixed order, no atomics.  Forward: the forward table, k_flip = 0.  Dgrad: in = grad_output and either
 *   the forward table of a submanifold map with k_flip = 1 or a reverse table (wcn_kmap_reverse) with k_flip = 0.
 * wcn_dwconv_wgrad: dw[k][c] = sum over the pairs p of bucket k of x[in_p][c] * dy[out_p][c]  (fp32 [K, C],
 *   overwritten, deterministic).  workspace: wcn_dwconv_wgrad_workspace(num_offsets, channels) bytes. */
int wcn_dwconv_gather(const void* in, const void* w, void* out, const int32_t* nbr, const float* bias, int64_t n_in,
                      int64_t n_out, int32_t channels, int32_t num_offsets, int32_t dtype, int32_t k_flip,
                      wcn_stream_t stream);
size_t wcn_dwconv_wgrad_workspace(int32_t num_offsets, int32_t channels);
int wcn_dwconv_wgrad(const void* x, const void* dy, float* dw, const int32_t* in_maps, const int32_t* out_maps,
                     const int32_t* offsets, int64_t n_in, int64_t n_out, int32_t channels, int32_t num_offsets,
                     int32_t dtype, void* workspace, size_t workspace_bytes, wcn_stream_t stream);

/* ---- point-cloud front end (PointConv path) ----------------------------------------------------------------------------
 * wcn_knn_grid: exact k nearest reference points of every query (k <= 64), ascending by distance.  The caller bins the
 *   reference points of ONE batch element into a uniform grid: cell = floor((p - origin) / cell_size) clamped to dims,
 *   cell id = (z * dims[1] + y) * dims[0] + x; `ref_sorted` [N,3] fp32 holds the points sorted by cell id, `ref_ids` [N]
 *   their original row ids, `cell_start` [cells + 1] the CSR over cells.  out_index [M,k] int64 (-1 if fewer than k
 *   points exist), out_dist2 [M,k] fp32 squared distances (may be NULL).  Equals the brute-force answer (up to ties);
 *   replaces the chunked cdist + topk of warpconvnet/geometry/coords/search/knn.py:11-26, 108-142.
 * wcn_segment_reduce: out[m][c] = op over rows [row_splits[m], row_splits[m+1]) of in[.][c], op: 0 sum, 1 mean, 2 max,
 *   3 min (empty segment -> 0); arg_rows [M,C] int64 (max / min only, may be NULL) = row of the first extremum, for the
 *   backward pass.  Role of torch_scatter.segment_csr in warpconvnet/ops/reductions.py:36-75. */
int wcn_knn_grid(const float* ref_sorted, const int32_t* ref_ids, const int32_t* cell_start, const float origin[3],
                 float cell_size, const int32_t dims[3], const float* query, int64_t num_query, int32_t k,
                 int64_t* out_index, float* out_dist2, wcn_stream_t stream);
/* Radius search over the same cell layout (cell_size >= radius, so the 27 cells around a query hold every point within
 * the radius; test `dist^2 <= radius^2`).  Two passes like the reference (warpconvnet/csrc/radius_search_kernels.cu:30-134,
 * call site geometry/coords/search/radius.py:16-124): wcn_radius_grid_count writes counts [M] int32; the caller scans them
 * into splits [M+1] int64 (device) and sizes the outputs; wcn_radius_grid_write fills out_index [total] int32 (original row
 * ids) and out_dist [total] fp32 distances (may be NULL).  Rows are in cell-walk order, deterministic. */
int wcn_radius_grid_count(const float* ref_sorted, const int32_t* ref_ids, const int32_t* cell_start, const float origin[3],
                          float cell_size, const int32_t dims[3], const float* query, int64_t num_query, float radius,
                          int32_t* counts, wcn_stream_t stream);
int wcn_radius_grid_write(const float* ref_sorted, const int32_t* ref_ids, const int32_t* cell_start, const float origin[3],
                          float cell_size, const int32_t dims[3], const float* query, int64_t num_query, float radius,
                          const int64_t* splits, int32_t* out_index, float* out_dist, wcn_stream_t stream);
int wcn_segment_reduce(const void* in, const int64_t* row_splits, int64_t num_segments, int32_t channels, int32_t dtype,
                       int32_t op, void* out, int64_t* arg_rows, wcn_stream_t stream);

/* ---- PointConv edge pipeline in one pass ----------------------------------------------------------------------------
 * Replaces the op sequence of warpconvnet/nn/modules/point_conv.py:231-273 (features[neighbors] / repeat_interleave / cat
 * -> edge_transform_mlp -> row_reduction) for the default edge MLP of warpconvnet/nn/modules/mlp.py:124-177
 * (Linear - LayerNorm - ReLU - Linear - LayerNorm + identity or Linear shortcut): for query q and its k neighbours j (uniform k, a
 * power of two <= 32, `nbr` [n_query * k] int32 rows of in_feats):
 *     x = [in_feats[j] | q_feats[q] | in_xyz[j] - q_xyz[q] (nrel = 3, else 0)],   out[q] = sum or mean over j of
 *     LN2(W2 ReLU(LN1(W1 x + b1)) + b2) + (x  or  Ws x + bs)     fp32, matrix cores (v_mfma_f32_32x32x2_f32).
 * No [n_query * k, C] tensor is written to HBM in either direction; the backward recomputes the chain per 32-edge tile.
 * wcn_pointconv_supported: cin + cq + nrel == cout unless linear_shortcut, and the widths fit an instantiated tile
 *   (edge-in <= 64, hidden <= 128, cout <= 64; smaller widths run zero-padded).
 * wcn_pointconv_pack: torch-layout parameters (w1 [hidden][ein], w2 [cout][hidden], biases / LayerNorm weights may be
 *   NULL = 0; ws [cout][ein] / bs = the Linear shortcut or NULL) -> operand images, wcn_pointconv_packed_floats floats.
 * wcn_pointconv_edge_backward: d_in [n_in][cin] must be ZERO-FILLED by the caller (neighbour rows are accumulated with
 *   hardware fp32 atomics: the one non-deterministic sum of the path, like index_add in the reference's autograd);
 *   d_q [n_query][cq] is written; d_params (wcn_pointconv_grad_floats floats) = dW1 [hidden][ein] | db1 | dLN1.weight |
 *   dLN1.bias | dW2 [cout][hidden] | db2 | dLN2.weight | dLN2.bias (| dWs [cout][ein] | dbs with a Linear shortcut),
 *   reduced over the workgroups in fixed order. */
int wcn_pointconv_supported(int32_t cin, int32_t cq, int32_t nrel, int32_t hidden, int32_t cout, int32_t k,
                            int32_t linear_shortcut);
int64_t wcn_pointconv_packed_floats(int32_t ein, int32_t hidden, int32_t cout);
int64_t wcn_pointconv_grad_floats(int32_t ein, int32_t hidden, int32_t cout, int32_t linear_shortcut);
size_t wcn_pointconv_backward_workspace(int64_t n_query, int32_t k, int32_t ein, int32_t hidden, int32_t cout,
                                        int32_t linear_shortcut);
int wcn_pointconv_pack(const float* w1, const float* b1, const float* g1, const float* be1, const float* w2,
                       const float* b2, const float* g2, const float* be2, const float* ws, const float* bs, int32_t ein,
                       int32_t hidden, int32_t cout, float* packed, wcn_stream_t stream);
int wcn_pointconv_edge_forward(const float* in_feats, const float* q_feats, const float* in_xyz, const float* q_xyz,
                               const int32_t* nbr, int64_t n_query, int32_t k, int32_t cin, int32_t cq, int32_t nrel,
                               const float* packed, int32_t hidden, int32_t cout, float eps1, float eps2, int32_t mean,
                               int32_t linear_shortcut, float* out, wcn_stream_t stream);
int wcn_pointconv_edge_backward(const float* in_feats, const float* q_feats, const float* in_xyz, const float* q_xyz,
                                const int32_t* nbr, int64_t n_query, int32_t k, int32_t cin, int32_t cq, int32_t nrel,
                                const float* packed, int32_t hidden, int32_t cout, float eps1, float eps2, int32_t mean,
                                int32_t linear_shortcut, const float* grad_out, float* d_in, float* d_q, float* d_params,
                                void* workspace, size_t workspace_bytes, wcn_stream_t stream);
/* Bitwise-reproducible variant (uniform lists): per-EDGE input gradients d_edge [n_query * k][cin] by plain stores instead of
 * the fp32 atomics on d_in; the caller sums the rows of each input point in a fixed order.  Used when the framework asks
 * for deterministic algorithms; reference: autograd of `features[neighbors]` (point_conv.py:243-246) is an index_add. */
int wcn_pointconv_edge_backward_peredge(const float* in_feats, const float* q_feats, const float* in_xyz, const float* q_xyz,
                                        const int32_t* nbr, int64_t n_query, int32_t k, int32_t cin, int32_t cq, int32_t nrel,
                                        const float* packed, int32_t hidden, int32_t cout, float eps1, float eps2, int32_t mean,
                                        int32_t linear_shortcut, const float* grad_out, float* d_edge, float* d_q,
                                        float* d_params, void* workspace, size_t workspace_bytes, wcn_stream_t stream);

/* The same pipeline over RAGGED neighbour lists (radius search, warpconvnet/geometry/coords/search/radius.py): `nbr`
 * [n_edges] = the lists of the queries behind each other, `edge_q` [n_edges] the query of every edge (non-decreasing, i.e.
 * repeat_interleave(arange(n_query), list lengths)), `q_scale` [n_query] the reduction scale per query (1 / length for mean,
 * NULL = sum).  `out` (forward) and `d_q` (backward) must be ZERO-FILLED by the caller: a list may straddle two 32-edge
 * tiles, so list segments are added to their rows (hardware fp32 atomics).  Workspace: wcn_pointconv_backward_workspace
 * (n_edges, 1, ...). */
int wcn_pointconv_edge_forward_ragged(const float* in_feats, const float* q_feats, const float* in_xyz, const float* q_xyz,
                                      const int32_t* nbr, const int32_t* edge_q, const float* q_scale, int64_t n_edges,
                                      int64_t n_query, int32_t cin, int32_t cq, int32_t nrel, const float* packed,
                                      int32_t hidden, int32_t cout, float eps1, float eps2, int32_t linear_shortcut,
                                      float* out, wcn_stream_t stream);
int wcn_pointconv_edge_backward_ragged(const float* in_feats, const float* q_feats, const float* in_xyz, const float* q_xyz,
                                       const int32_t* nbr, const int32_t* edge_q, const float* q_scale, int64_t n_edges,
                                       int64_t n_query, int32_t cin, int32_t cq, int32_t nrel, const float* packed,
                                       int32_t hidden, int32_t cout, float eps1, float eps2, int32_t linear_shortcut,
                                       const float* grad_out, float* d_in, float* d_q, float* d_params, void* workspace,
                                       size_t workspace_bytes, wcn_stream_t stream);

/* Sparse pooling over a kernel map (REDUCE_AND_STRIDE, SparsePool / SparseMaxPool / SparseUnpool): out[m][c] =
 * reduce over the present neighbours k of in[tbl[m][k]][c]; `tbl` is the row-major neighbour table [n_out][row pitch of
 * num_offsets] (-1 = absent) that wcn_kmap_probe / wcn_kmap_from_csr / wcn_kmap_reverse produce.  op: 0 sum, 1 mean,
 * 2 max, 3 min; rows without a neighbour give 0.  `arg` (may be NULL) int32 [n_out][channels] = winning input row of
 * max / min (first extremum in offset order, -1 if none); `count` (may be NULL) int32 [n_out] = neighbours per row.
 * One pass, no intermediate tensors; replaces to_csr + index gather + torch_scatter.segment_csr
 * (warpconvnet/nn/functional/sparse_pool.py:84-110). */
int wcn_pool_gather(const void* in, const int32_t* tbl, int64_t n_in, int64_t n_out, int32_t channels, int32_t num_offsets,
                    int32_t dtype, int32_t op, void* out, int32_t* arg, int32_t* count, wcn_stream_t stream);
/* The same over in[r][c] * scale[r]: `scale` fp32 [n_in], one factor per SOURCE row (NULL = wcn_pool_gather).  The
 * backward of the mean runs it over the reverse table with scale = 1 / count: the terms dy[r] / count[r] are formed and
 * summed in fp32 and the sum is rounded once.  Both entry points take the 16-B row pieces only when `in` and `out` are
 * 16-B aligned (and channels is a whole number of pieces) and one element at a time otherwise; wcn_pool_select does the
 * same for `dy` and `dx`.  Pointers must be aligned to their element. */
int wcn_pool_gather_scaled(const void* in, const int32_t* tbl, const float* scale, int64_t n_in, int64_t n_out,
                           int32_t channels, int32_t num_offsets, int32_t dtype, int32_t op, void* out, int32_t* arg,
                           int32_t* count, wcn_stream_t stream);
/* Host only: elements per memory access the pooling kernels use for feature pointers `src` and `dst` (nothing is
 * dereferenced): 16 / element size, or 1 when channels is no whole number of 16-B pieces or a pointer is not 16-B aligned;
 * 0 for a bad dtype or channels < 1. */
int wcn_pool_row_vec(const void* src, const void* dst, int32_t channels, int32_t dtype);
/* Gradient of max / min pooling, output-stationary and deterministic: dx[n][c] = sum over the present k of
 * dy[r][c] where r = tbl[n][k] and arg[r][c] == n.  `tbl` is the REVERSE table [n_in][pitch] (pooled rows per input
 * row), `arg` the forward pass's [n_out][channels]. */
int wcn_pool_select(const void* dy, const int32_t* arg, const int32_t* tbl, int64_t n_in, int64_t n_out, int32_t channels,
                    int32_t num_offsets, int32_t dtype, void* dx, wcn_stream_t stream);

/* ---- BatchNorm over sparse feature tensors [n, channels] (f32 / f16 / bf16 storage, fp32 statistics) --------------------
 * The elementwise chain behind every sparse convolution (reference models/mink_unet.py:31-53: SparseConv3d ->
 * nn.BatchNorm1d -> ReLU, the framework's stock BatchNorm kernels).  All passes stream the tensor once; the two
 * reductions are fixed-order two-level sums (deterministic).  `workspace` >= wcn_bn_workspace(channels) bytes.
 *   wcn_bn_stats            mean[c], var[c] (biased, /n) in one pass (sums around the pivot x[0][c]).
 *   wcn_bn_apply            y = x * scale[c] + shift[c]; relu != 0: max(., 0).  (training: scale = gamma * rstd,
 *                           shift = beta - mean * scale; inference: the same from the running statistics.)
 *   wcn_bn_backward_reduce  sum_dy[c] = sum_r g, sum_dy_xhat[c] = sum_r g * (x - mean) * rstd, where g = dy, or 0 where the
 *                           fused ReLU of the forward pass stored a zero: `relu_scale` / `relu_shift` (both or neither) are the
 *                           scale / shift the forward applied, the mask is recomputed from x with the same fused
 *                           multiply-add and rounding - the forward output is not read again.
 *   wcn_bn_backward_apply   dx = gamma * rstd * (g - sum_dy / n - xhat * sum_dy_xhat / n); gamma may be NULL (= 1). */
size_t wcn_bn_workspace(int32_t channels);
/* Widest layer the BatchNorm passes take (3276: the backward apply stages five fp32 coefficients per channel in 64 KB of LDS).
 * Every wcn_bn_* entry below (and wcn_conv_bn_backward* through them) returns WCN_ERROR_UNSUPPORTED_CONFIG for `channels`
 * above it, before any launch and whatever else is wrong with the arguments - forward and backward alike, so that a layer whose
 * forward ran cannot fail in its backward. */
int32_t wcn_bn_max_channels(void);
/*   wcn_bn_stats_fold       wcn_bn_stats plus, in the same launches, everything a training step derives from the
 *                           statistics: rstd = 1/sqrt(var + eps), scale = gamma * rstd, shift = beta - mean * scale (gamma /
 *                           beta may be NULL) and the in-place update of the fp32 running statistics (NULL: none) with
 *                           `momentum` and the unbiased variance - the ~10 tiny framework kernels of a BatchNorm step;
 *                           `num_batches_tracked` (device int64 scalar, NULL: none) is incremented by one.
 *   wcn_bn_fold             inference: mean / rstd / scale / shift from the running statistics, one launch. */
int wcn_bn_stats_fold(const void* x, int64_t n, int32_t channels, int32_t dtype, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, float momentum, float eps, float* mean, float* var,
                      float* rstd, float* scale, float* shift, int64_t* num_batches_tracked, void* workspace,
                      size_t workspace_bytes, wcn_stream_t stream);
int wcn_bn_fold(const float* running_mean, const float* running_var, const float* gamma, const float* beta, float eps,
                int32_t channels, float* mean, float* rstd, float* scale, float* shift, wcn_stream_t stream);
int wcn_bn_stats(const void* x, int64_t n, int32_t channels, int32_t dtype, float* mean, float* var, void* workspace,
                 size_t workspace_bytes, wcn_stream_t stream);
int wcn_bn_apply(const void* x, int64_t n, int32_t channels, int32_t dtype, const float* scale, const float* shift,
                 int32_t relu, void* y, wcn_stream_t stream);
int wcn_bn_backward_reduce(const void* dy, const void* x, const float* relu_scale, const float* relu_shift, int64_t n,
                           int32_t channels, int32_t dtype, const float* mean, const float* rstd, float* sum_dy,
                           float* sum_dy_xhat, void* workspace, size_t workspace_bytes, wcn_stream_t stream);
int wcn_bn_backward_apply(const void* dy, const void* x, const float* relu_scale, const float* relu_shift, int64_t n,
                          int32_t channels, int32_t dtype, const float* mean, const float* rstd, const float* gamma,
                          const float* sum_dy, const float* sum_dy_xhat, void* dx, wcn_stream_t stream);
/* The tail of a residual block, z = ReLU(BN(x) + r) - the reference runs it as three passes over the feature tensor
 * (`models/mink_unet.py:160-172`: conv2's BatchNorm, `out += identity`, `relu(out)`).  Here it rides on the two BatchNorm passes:
 *   wcn_bn_apply_residual          y = [ReLU](round(x * scale + shift) + residual), every intermediate rounded to the storage
 *                                  type as the three modules would (bit-identical to them).
 *   wcn_bn_backward_reduce_masked  as wcn_bn_backward_reduce with g = dy where the stored output z is positive, else 0.
 *   wcn_bn_backward_apply_masked   as wcn_bn_backward_apply with that mask; `dres` (may be NULL) also receives g itself -
 *                                  the gradient of the residual branch. */
int wcn_bn_apply_residual(const void* x, const void* residual, int64_t n, int32_t channels, int32_t dtype, const float* scale,
                          const float* shift, int32_t relu, void* y, wcn_stream_t stream);
int wcn_bn_backward_reduce_masked(const void* dy, const void* x, const void* z, int64_t n, int32_t channels, int32_t dtype,
                                  const float* mean, const float* rstd, float* sum_dy, float* sum_dy_xhat, void* workspace,
                                  size_t workspace_bytes, wcn_stream_t stream);
int wcn_bn_backward_apply_masked(const void* dy, const void* x, const void* z, int64_t n, int32_t channels, int32_t dtype,
                                 const float* mean, const float* rstd, const float* gamma, const float* sum_dy,
                                 const float* sum_dy_xhat, void* dx, void* dres, wcn_stream_t stream);

/* Layer entries: the BatchNorm of a training step in ONE call per direction (the host side of a network pays per call, not per
 * launch: tools/host_attrib.py).  `stats` [5][channels] fp32 = mean | rstd | scale | shift | biased variance, written by the
 * forward and read by the backward.  wcn_bn_train_forward = wcn_bn_stats_fold + wcn_bn_apply[_residual] (`residual` may be NULL);
 * wcn_bn_train_backward = wcn_bn_backward_reduce[_masked] + wcn_bn_backward_apply[_masked]: `z` (stored output of a residual
 * tail, its sign is the ReLU mask) or NULL (mask recomputed from x when `relu`), `sums` [2][channels] = sum_dy | sum_dy_xhat,
 * `dx` NULL = sums only, `dres` (masked gradient, residual tails) may be NULL, `training` 0 = statistics were constants. */
int wcn_bn_train_forward(const void* x, const void* residual, int64_t n, int32_t channels, int32_t dtype, const float* gamma,
                         const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                         int64_t* num_batches_tracked, int32_t relu, float* stats, void* y, void* workspace,
                         size_t workspace_bytes, wcn_stream_t stream);
int wcn_bn_train_backward(const void* dy, const void* x, const void* z, int32_t relu, int64_t n, int32_t channels, int32_t dtype,
                          const float* stats, const float* gamma, int32_t training, float* sums, void* dx, void* dres,
                          void* workspace, size_t workspace_bytes, wcn_stream_t stream);
/* The same with a row pitch for `dy` (elements; >= channels, 0 = channels): the gradient a channel concatenation hands to one of
 * its inputs is a column slice of a wider row-major tensor (reference models/mink_unet.py:392-404: `cat` of the up-sampled and
 * the skip tensor) - read in place instead of through a contiguous copy.  16-B pieces need dy and dy_ld * sizeof(T) 16-B
 * aligned; anything else takes the element path. */
int wcn_bn_train_backward_ld(const void* dy, int64_t dy_ld, const void* x, const void* z, int32_t relu, int64_t n, int32_t channels,
                             int32_t dtype, const float* stats, const float* gamma, int32_t training, float* sums, void* dx,
                             void* dres, void* workspace, size_t workspace_bytes, wcn_stream_t stream);

/* Layer entry: backward of SparseConv3d -> BatchNorm (-> ReLU | residual tail) (reference models/mink_unet.py:31-53, 160-172 run
 * as three autograd nodes) in one call: wcn_bn_train_backward into `dy_conv` ([n_out][cout], caller's buffer), then
 * wcn_conv_gather_gemm on the reverse tables with the transposed packed weight (`dx` NULL: skipped), then wcn_conv_wgrad (`dw`
 * NULL: skipped).  16-bit dtypes, MFMA shapes (wcn_mfma_gather_supported in both directions, wcn_mfma_wgrad_supported). */
int wcn_conv_bn_backward(const void* grad_out, const void* x, const void* y, const void* z, int32_t relu, const float* stats,
                         const float* gamma, int32_t training, float* sums, void* dy_conv, void* dres, const void* w_packed_dgrad,
                         const int32_t* rev_nbr, const uint32_t* rev_mask, const int32_t* rev_perm, int32_t flip, void* dx,
                         const int32_t* in_maps, const int32_t* out_maps, const int32_t* offsets, float* dw, void* wgrad_workspace,
                         size_t wgrad_workspace_bytes, int64_t n_in, int64_t n_out, int32_t cin, int32_t cout, int32_t num_offsets,
                         int32_t dtype, void* bn_workspace, size_t bn_workspace_bytes, wcn_stream_t stream);
/* ... with a row pitch for `grad_out` (see wcn_bn_train_backward_ld). */
int wcn_conv_bn_backward_ld(const void* grad_out, int64_t grad_out_ld, const void* x, const void* y, const void* z, int32_t relu,
                            const float* stats, const float* gamma, int32_t training, float* sums, void* dy_conv, void* dres,
                            const void* w_packed_dgrad, const int32_t* rev_nbr, const uint32_t* rev_mask, const int32_t* rev_perm,
                            int32_t flip, void* dx, const int32_t* in_maps, const int32_t* out_maps, const int32_t* offsets,
                            float* dw, void* wgrad_workspace, size_t wgrad_workspace_bytes, int64_t n_in, int64_t n_out,
                            int32_t cin, int32_t cout, int32_t num_offsets, int32_t dtype, void* bn_workspace,
                            size_t bn_workspace_bytes, wcn_stream_t stream);

/* ... with the map's slab bounds (wcn_kmap_slab_bounds_offset; NULL = none) for the weight gradient: the sweep of
 * wcn_conv_wgrad_teams on the same operands, so a layer computes the same bits through this entry and through the passes one by one. */
int wcn_conv_bn_backward_teams(const void* grad_out, int64_t grad_out_ld, const void* x, const void* y, const void* z, int32_t relu,
                               const float* stats, const float* gamma, int32_t training, float* sums, void* dy_conv, void* dres,
                               const void* w_packed_dgrad, const int32_t* rev_nbr, const uint32_t* rev_mask,
                               const int32_t* rev_perm, int32_t flip, void* dx, const int32_t* in_maps, const int32_t* out_maps,
                               const int32_t* offsets, const int32_t* slab_bounds, float* dw, void* wgrad_workspace,
                               size_t wgrad_workspace_bytes, int64_t n_in, int64_t n_out, int32_t cin, int32_t cout,
                               int32_t num_offsets, int32_t dtype, void* bn_workspace, size_t bn_workspace_bytes,
                               wcn_stream_t stream);

/* ---- block-diagonal ("varlen") multi-head attention over a packed qkv tensor ----------------------------------------------
 * The attention core of PatchAttention (reference nn/modules/attention.py:496 calls flash_attn_varlen_qkvpacked_func through
 * nn/functional/flash_attn_utils.py:15-82); same contract without dropout, causal mask or window.  `qkv` [total, 3, heads,
 * head_dim] contiguous (slot 0 = Q, 1 = K, 2 = V), `cu_seqlens` int32 [num_seqs + 1], device: sequence s is the rows
 * [cu[s], cu[s+1]), a row attends to the rows of its own sequence only.  `max_seqlen` >= every length (it sizes the grid; the
 * host never reads cu_seqlens).  Rows outside every sequence are not written.
 *   wcn_attn_varlen_supported        host-only: 1 if head_dim in {16, 32, 64} and dtype is WCN_F16 / WCN_BF16.
 *   wcn_attn_varlen_workspace_bytes  host-only: the backward's fp32 [total, heads] workspace (delta = rowsum(dO * O)).
 *   wcn_attn_varlen_fwd              out [total, heads, head_dim] (dtype), lse [total, heads] fp32 = ln sum_k exp(scale q.k).
 *   wcn_attn_varlen_bwd              dqkv [total, 3, heads, head_dim] (dtype) from dout / out [total, heads, head_dim] and the
 *                                    forward's lse; every row of every sequence written exactly once, fixed-order sums (two
 *                                    calls give bit-identical dqkv).
 * Arguments are checked before any launch: unsupported head_dim / dtype -> WCN_ERROR_UNSUPPORTED_CONFIG; heads < 1,
 * max_seqlen < 0, negative sizes, null pointers with total > 0, a short workspace -> WCN_ERROR_INVALID_PARAMETERS. */
int wcn_attn_varlen_supported(int32_t head_dim, int32_t dtype);
size_t wcn_attn_varlen_workspace_bytes(int64_t total, int32_t heads);
int wcn_attn_varlen_fwd(const void* qkv, const int32_t* cu_seqlens, int64_t num_seqs, int64_t total, int32_t heads,
                        int32_t head_dim, int32_t max_seqlen, float softmax_scale, int32_t dtype, void* out, float* lse,
                        wcn_stream_t stream);
int wcn_attn_varlen_bwd(const void* dout, const void* qkv, const void* out, const float* lse, const int32_t* cu_seqlens,
                        int64_t num_seqs, int64_t total, int32_t heads, int32_t head_dim, int32_t max_seqlen,
                        float softmax_scale, int32_t dtype, void* dqkv, void* workspace, size_t workspace_bytes,
                        wcn_stream_t stream);

/* ---- varlen attention with separate Q and K/V operands: cross-attention (ABI 10, additions only) ------------------------------
 * The attention core of the reference's SparseMultiHeadAttention(type="cross") (nn/modules/sparse_dit_attention.py:265-315 calls
 * flash_attn.flash_attn_varlen_func / flash_attn_varlen_kvpacked_func); same contract without dropout, causal mask or window,
 * and the same kernels as the packed form above (which calls them with the three slots of its one tensor).
 * `q` [total_q] rows of heads * head_dim elements, `q_stride` elements apart; `k`, `v` [total_k] rows with ONE common stride
 * `kv_stride` (a kv-packed [total_k, 2, heads, head_dim] tensor: v = k + heads * head_dim, kv_stride = 2 * heads * head_dim).
 * `cu_q`, `cu_k` int32 [num_seqs + 1], device: sequence s is the queries [cu_q[s], cu_q[s+1]) against the keys
 * [cu_k[s], cu_k[s+1]).  `max_seqlen_q` / `max_seqlen_k` >= every length of their side (they size the grids; the host never
 * reads cu_*).  `out`, `dout` [total_q, heads, head_dim] and `lse` [total_q, heads] fp32 are contiguous; `dq` has the row
 * stride `dq_stride`, `dk` and `dv` ONE common stride `dkv_stride`.  Rows outside every sequence are not written; every row
 * of every sequence is written exactly once in each of out, lse, dq, dk, dv.
 * Empty sides: a query of a sequence with no key gets out = 0 and lse = -inf, and dq = 0 in the backward; the keys of a
 * sequence with no query get dk = dv = 0 (exact zeros, never NaN).
 * The dK/dV pass is one wave per (sequence, 32-key block, head) sweeping the sequence's query blocks.  `q_splits` > 1 cuts that
 * sweep into q_splits contiguous shares, each wave writing fp32 partials [q_splits, total_k, 2, heads, head_dim] into the
 * workspace; a second kernel adds the splits in the fixed order 0 .. q_splits - 1, scales, casts and stores.  q_splits = 1
 * stores directly and touches no partials.  Any q_splits gives bit-identical results across calls; dq does not depend on it.
 *   wcn_attn_varlen_kv_splits           host-only: the split count the library chooses for q_splits = 0, >= 1, from these
 *                                       numbers alone: enough splits for about 4096 waves, at least 16 query blocks of
 *                                       max_seqlen_q per split, at most 16 splits, and never more than fit a partial workspace
 *                                       of 256 MiB at num_seqs * max_seqlen_k keys and head_dim 64.
 *   wcn_attn_varlen_kv_workspace_bytes  host-only: delta fp32 [total_q, heads] = 4 * total_q * heads bytes, plus, when
 *                                       q_splits > 1, the partials 4 * q_splits * total_k * 2 * heads * head_dim bytes.
 *   wcn_attn_varlen_kv_fwd              out, lse.
 *   wcn_attn_varlen_kv_bwd              dq, dk, dv from dout / out and the forward's lse.  q_splits = 0: choose as
 *                                       wcn_attn_varlen_kv_splits does; the workspace must hold what
 *                                       wcn_attn_varlen_kv_workspace_bytes reports for the count in use.
 * Arguments are checked before any launch: unsupported head_dim / dtype -> WCN_ERROR_UNSUPPORTED_CONFIG; heads < 1, negative
 * sizes or max_seqlen_*, total_q or total_k > INT32_MAX, a stride that is not a multiple of 8 elements or shorter than a row,
 * a base pointer (q, k, v, out, dout, dq, dk, dv, workspace) that is not 16-byte aligned, null pointers with rows to process,
 * q_splits < 0, a short workspace -> WCN_ERROR_INVALID_PARAMETERS. */
int32_t wcn_attn_varlen_kv_splits(int64_t num_seqs, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t heads);
size_t wcn_attn_varlen_kv_workspace_bytes(int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim, int32_t q_splits);
int wcn_attn_varlen_kv_fwd(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                           const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs, int64_t total_q, int64_t total_k,
                           int32_t heads, int32_t head_dim, int32_t max_seqlen_q, int32_t max_seqlen_k, float softmax_scale,
                           int32_t dtype, void* out, float* lse, wcn_stream_t stream);
int wcn_attn_varlen_kv_bwd(const void* dout, const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                           const void* out, const float* lse, const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs,
                           int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim, int32_t max_seqlen_q,
                           int32_t max_seqlen_k, float softmax_scale, int32_t dtype, void* dq, int64_t dq_stride, void* dk,
                           void* dv, int64_t dkv_stride, int32_t q_splits, void* workspace, size_t workspace_bytes,
                           wcn_stream_t stream);

/* ---- sparse resampling over a CHILD TABLE (ABI 6, additions only) -----------------------------------------------------------
 * Space-to-channel / channel-to-space / subdivide / up- and down-sampling / prune of sparse VAEs and generative decoders
 * (reference, pure torch: nn/modules/sparse_resample.py:44-287, nn/modules/prune.py, nn/functional/sparse_ops.py:33-65).
 * `tbl` [n_parent][pitch] int32: tbl[p][col] = the fine row that is a child of coarse row p, or -1; n_per = factor^3 children,
 * factor in {2, 3, 4} (and factor = n_per = 1: the compaction of prune); larger factors -> WCN_ERROR_UNSUPPORTED_CONFIG.
 * The CHANNEL slot of the child at (x, y, z) is the reference's s = (x mod f) + f (y mod f) + f^2 (z mod f)
 * (sparse_resample.py:202-203).  `slot_order` names the column order of the table: WCN_SLOT_X_FASTEST col = s (tables of
 * wcn_resample_expand), WCN_SLOT_Z_FASTEST col = ((x mod f) f + (y mod f)) f + (z mod f) - the kernel-offset order of
 * wcn_cells_stride_emit and of a kernel map with kernel_size == stride == f (pitch = wcn_kmap_row_pitch(n_per)).
 * Feature rows are `dtype` (f32 / f16 / bf16), any channels >= 1: 16-B pieces when channels * sizeof(T) is a multiple of 16 and
 * the buffers are 16-B aligned, single elements otherwise.  Pure copies: deterministic, no atomics, bit-exact.
 *   wcn_resample_pack    dst [n_parent][n_per * channels]: dst[p][s*C .. (s+1)*C) = src[tbl[p][col(s)]] or 0 where the child
 *                        is absent - ONE pass, the zeros are written by the same kernel (the reference fills zeros, then
 *                        scatters).  Forward of space-to-channel, backward of channel-to-space / prune.  src [n_src][channels].
 *   wcn_resample_unpack  dst [n_dst][channels]: dst[tbl[p][col(s)]] = src[p][s*C .. (s+1)*C) for every present child; rows of
 *                        dst no entry names are not written.  Forward of channel-to-space / prune, backward of
 *                        space-to-channel.  broadcast = 1: src is [n_parent][channels] and every child receives src[p] - the
 *                        feature side of up-sampling and subdivision; tbl = NULL: the dense subdivision, child s of p is row
 *                        p * n_per + s.
 *   wcn_resample_expand  the subdivision a mask describes.  parents [n_parent][4] (b, x, y, z), batch-sorted; mask
 *                        [n_parent][n_per], mask_dtype 0 / 1 / 2 = wcn_dtype ("non-zero = keep"), 3 = bytes (a bool tensor);
 *                        NULL = keep all.  Children are ordered by parent row, then ascending column; the child of column
 *                        j sits at factor * parent + (j % f, j / f % f, j / f^2) (WCN_SLOT_X_FASTEST) or
 *                        + (j / f^2, j / f % f, j % f) (WCN_SLOT_Z_FASTEST, the order of the reference's SparseSubdivide).
 *                        Two phases on one workspace (wcn_resample_expand_workspace(n_parent) bytes), selected by the
 *                        outputs given: out_offsets != NULL: count + exclusive scan, out_offsets [num_batches + 1] =
 *                        children of the parents with a batch index < b (the last entry is their number M: the ONE host
 *                        read); child_coords / tbl != NULL: emit child_coords [M][4] and tbl [n_parent][pitch] (col = mask
 *                        column) from the counts a phase-1 call left in the workspace; `capacity` = rows of child_coords,
 *                        nothing past it is written.  Both in one call when the caller sizes child_coords by the bound
 *                        n_parent * n_per. */
enum wcn_slot_order { WCN_SLOT_X_FASTEST = 0, WCN_SLOT_Z_FASTEST = 1 };
int wcn_resample_pack(const void* src, const int32_t* tbl, int64_t n_src, int64_t n_parent, int32_t channels, int32_t n_per,
                      int32_t factor, int32_t pitch, int32_t slot_order, int32_t dtype, void* dst, wcn_stream_t stream);
int wcn_resample_unpack(const void* src, const int32_t* tbl, int64_t n_parent, int64_t n_dst, int32_t channels, int32_t n_per,
                        int32_t factor, int32_t pitch, int32_t slot_order, int32_t broadcast, int32_t dtype, void* dst,
                        wcn_stream_t stream);
size_t wcn_resample_expand_workspace(int64_t n_parent);
int wcn_resample_expand(const int32_t* parents, const void* mask, int32_t mask_dtype, int64_t n_parent, int32_t n_per,
                        int32_t factor, int32_t slot_order, int32_t num_batches, void* workspace, size_t workspace_bytes,
                        int32_t* out_offsets, int64_t capacity, int32_t* child_coords, int32_t* tbl, int32_t pitch,
                        wcn_stream_t stream);

/* ---- Q/K prologue of sparse voxel self-attention: qk-RMSNorm, coordinate RoPE, cast (ABI 7, additions only) ------------------
 * What the reference's SparseMultiHeadAttention runs between `to_qkv` and the attention core
 * (nn/modules/sparse_dit_attention.py:249-262: unbind -> MultiHeadRMSNorm -> SparseRotaryPositionEmbedder -> stack) and its
 * fused rotation (nn/functional/fused_rope.py:30,55 -> csrc/fused_rope_kernel.cu), as one pass over `qkv` [total, 3, heads,
 * head_dim] contiguous (slot 0 = Q, 1 = K, 2 = V); head_dim even, <= 256.
 * The rotation: a head is head_dim / 2 pairs (x[2j], x[2j+1]); pair j < rot_pairs = 3 * num_freqs turns by the angle
 * pos[a] * freqs[f], a = j / num_freqs, f = j % num_freqs, pos[a] = float(coord[a]) - origin[a] + bias (fp32, one rounding
 * per operation); out = (x0 cos - x1 sin, x0 sin + x1 cos), `conjugate` = 1 negates sin (the inverse rotation).  Pairs
 * j >= rot_pairs and the whole V slot pass through.  The reference's two conventions are two settings: fused_rope_qkv is
 * origin = column minimum, bias = 1, freqs = theta; SparseRotaryPositionEmbedder is origin = NULL, bias = 0,
 * freqs[i] = f0 / f1^(i / F).
 *   wcn_rope_table                   table [total, 3 * num_freqs, 2] fp32 = (cos, sin), with the accurate sincosf.  `coords`
 *                                    [total, 3] int32 (coords_float = 0) or fp32 (1); `origin` device float[3] or NULL (= 0);
 *                                    `freqs` device float[num_freqs], 6 * num_freqs <= 256.
 *   wcn_qk_prologue_supported        host-only: 1 if head_dim is even, 2..256, in_dtype is f32 / f16 / bf16 and out_dtype
 *                                    f16 / bf16.
 *   wcn_qk_prologue_workspace_bytes  host-only: the backward's workspace (fp32 partial sums of the gamma gradients).
 *   wcn_qk_prologue_fwd              out [total, 3, heads, head_dim] (out_dtype: f16 / bf16; an f32 input is cast here).
 *                                    gamma_q, gamma_k [heads, head_dim] fp32, both or neither: each (token, head) of Q and
 *                                    K becomes x / max(|x|_2, 1e-12) * gamma[h] * sqrt(head_dim) in fp32, not rounded before
 *                                    the rotation, and inv_norm [total, 2, heads] fp32 = 1 / max(|x|_2, 1e-12) is written for
 *                                    the backward.  `table` NULL with rot_pairs = 0: no rotation.  Neither: a cast copy.
 *   wcn_qk_prologue_bwd              dqkv [total, 3, heads, head_dim] (in_dtype) from dout (dout_dtype: f16 / bf16).  Without
 *                                    gammas it is the forward on dout with conjugate = 1 (`qkv`, `inv_norm`, `dgamma_*`,
 *                                    `workspace` unused).  With them: dy = un-rotated dout, u = gamma sqrt(D) dy,
 *                                    xh = x inv_norm, dx = (u - xh (xh . u)) inv_norm (u * 1e12 where the norm was clamped),
 *                                    dgamma_q / dgamma_k [heads, head_dim] fp32 = sum_t sqrt(D) xh dy through per-row-group
 *                                    partial sums in `workspace` and a fixed-order second pass: no float atomics, two calls
 *                                    give bit-identical dqkv and dgamma.
 * 16-byte pieces per lane when head_dim is a multiple of 8 (f16 / bf16 on both sides) or 4 (an f32 side) and the buffers
 * are 16-B aligned, one pair per lane otherwise.  Arguments are checked before any launch: a dtype outside the above, an odd
 * head_dim or head_dim > 256 -> WCN_ERROR_UNSUPPORTED_CONFIG; negative sizes, heads < 1, 2 * rot_pairs > head_dim, one gamma
 * without the other, total * 3 * heads > INT32_MAX, null pointers with total > 0, a buffer not aligned to one pair, a short
 * workspace -> WCN_ERROR_INVALID_PARAMETERS; total == 0 -> WCN_SUCCESS without a launch. */
int wcn_rope_table(const void* coords, int32_t coords_float, int64_t total, const float* origin, float bias,
                   const float* freqs, int32_t num_freqs, float* table, wcn_stream_t stream);
int wcn_qk_prologue_supported(int32_t head_dim, int32_t in_dtype, int32_t out_dtype);
size_t wcn_qk_prologue_workspace_bytes(int64_t total, int32_t heads, int32_t head_dim);
int wcn_qk_prologue_fwd(const void* qkv, int32_t in_dtype, int64_t total, int32_t heads, int32_t head_dim, const float* table,
                        int32_t rot_pairs, int32_t conjugate, const float* gamma_q, const float* gamma_k, void* out,
                        int32_t out_dtype, float* inv_norm, wcn_stream_t stream);
int wcn_qk_prologue_bwd(const void* dout, int32_t dout_dtype, const void* qkv, int32_t in_dtype, int64_t total, int32_t heads,
                        int32_t head_dim, const float* table, int32_t rot_pairs, const float* gamma_q, const float* gamma_k,
                        const float* inv_norm, void* dqkv, float* dgamma_q, float* dgamma_k, void* workspace,
                        size_t workspace_bytes, wcn_stream_t stream);

/* ---- adaLN modulation and gated residual of a sparse transformer block (ABI 8, additions only) ------------------------------
 * The per-voxel glue of the reference's ModulatedSparseTransformerBlock (nn/modules/sparse_dit.py:108-123, a dozen
 * element-wise torch passes per branch) as one streaming pass per direction.  With b = the segment of row t
 * (cu[b] <= t < cu[b+1]; `cu` int32 [num_segs + 1] on the device, empty segments allowed, never read on the host):
 *     x1 = x + h * gate[b]                            with `h` and `gate`   (NULL, NULL: x1 = x, nothing written)
 *     y  = LN(x1) * (1 + scale[b]) + shift[b]         with `shift` and `scale` (NULL, NULL: no y)
 * LN has no affine parameters, the biased variance and `eps`.  `x`, `h`, `x1`, `y` are [rows, channels] contiguous in
 * `dtype` (f32 / f16 / bf16); `gate`, `shift`, `scale` are fp32 [num_segs, channels] views with the common row pitch
 * `mod_ld` floats (chunks of one [num_segs, 6 * channels] tensor).  All arithmetic is fp32 with one rounding to the output
 * dtype: y comes from the fp32 x1, not from its rounded value; the variance is two-pass (mean, then squared deviations).
 *   wcn_adaln_supported        host-only: 1 if channels is a multiple of 8 in 8..2048 and dtype is f32 / f16 / bf16.
 *   wcn_adaln_workspace_bytes  host-only: the backward's workspace, (ceil(rows / 64) + num_segs) * 3 * channels floats.
 *   wcn_adaln_fwd              writes x1 (with h, gate), y and stats [rows, 2] fp32 = (mean, rstd) (with shift, scale).
 *   wcn_adaln_bwd              `dy` (with `scale`, `stats` and the forward's `x`) selects the norm, `h` (with `gate`) the
 *                              gated residual; `dx1` = the gradient that reaches x1 directly, or NULL (required without
 *                              dy).  x1 = x + h gate[b] is formed again in fp32 (the forward's bits, not its rounded
 *                              output), xhat = (x1 - mean) rstd, g = dy (1 + scale[b]):
 *                                  dx = dx1 + rstd (g - mean_c(g) - xhat mean_c(g xhat))      (`dx` may be NULL without dy)
 *                                  dh = dx gate[b],   dgate[b] = sum_{t in b} dx h,
 *                                  dshift[b] = sum_{t in b} dy,   dscale[b] = sum_{t in b} dy xhat
 *                              dgate / dshift / dscale fp32 [num_segs, channels] with the row pitch `dmod_ld`, zeros for a
 *                              segment without rows.  The sums go through per-(64-row chunk, segment) partial slots in
 *                              `workspace` and a fixed-order second pass: no float atomics, two calls give bit-identical
 *                              results.
 * Arguments are checked before any launch: channels / dtype outside the above -> WCN_ERROR_UNSUPPORTED_CONFIG; negative
 * sizes, rows > INT32_MAX, neither use selected, one pointer of a pair without the other, a pointer the selected use needs
 * missing, mod_ld / dmod_ld < channels, mod_ld not a multiple of 4, a short workspace, row buffers / mod views / workspace
 * not 16-B aligned -> WCN_ERROR_INVALID_PARAMETERS.  rows == 0 or num_segs == 0 -> WCN_SUCCESS without a kernel (the
 * backward still zero-fills dgate / dshift / dscale); the use is still told from the pointers, so a caller whose empty
 * buffers have no address decides these cases itself. */
int wcn_adaln_supported(int32_t channels, int32_t dtype);
size_t wcn_adaln_workspace_bytes(int64_t rows, int64_t num_segs, int32_t channels);
int wcn_adaln_fwd(const void* x, const void* h, const float* gate, const float* shift, const float* scale, int64_t mod_ld,
                  const int32_t* cu, int64_t num_segs, int64_t rows, int32_t channels, float eps, int32_t dtype, void* x1,
                  void* y, float* stats, wcn_stream_t stream);
int wcn_adaln_bwd(const void* dx1, const void* dy, const void* x, const void* h, const float* gate, const float* scale,
                  int64_t mod_ld, const float* stats, const int32_t* cu, int64_t num_segs, int64_t rows, int32_t channels,
                  int32_t dtype, void* dx, void* dh, float* dgate, float* dshift, float* dscale, int64_t dmod_ld,
                  void* workspace, size_t workspace_bytes, wcn_stream_t stream);

/* ---- LayerNorm (+ affine) (+ SiLU) and the channel spread / fold of the sparse U-Net blocks (ABI 9, additions only) ---------
 * The per-voxel glue of the reference's residual blocks (nn/modules/sparse_unet.py: norm(x.float()).to(dtype) -> silu between
 * two convolutions, five or six [N, C] torch passes per site; h + repeat_interleave(x) / h + reshape(...).mean(-1) at the end)
 * as one streaming pass per site and direction.
 *     xhat = (x - mean) * rstd           biased variance, `eps`, fp32, two-pass (mean, then squared deviations)
 *     z    = xhat * weight + bias        with `weight` and `bias` (NULL, NULL: z = xhat)
 *     y    = act ? z * sigmoid(z) : z    `act` 0 = none, 1 = SiLU; rounded once, to `dtype`
 * `x`, `y`, `dy`, `dx` are [rows, channels] contiguous in `dtype` (f32 / f16 / bf16); `weight`, `bias` fp32 [channels].
 *   wcn_ln_act_supported        host-only: the domain of wcn_adaln_supported (channels a multiple of 8 in 8..2048).
 *   wcn_ln_act_workspace_bytes  host-only: the backward's workspace with weight / bias, ceil(rows / 64) * 2 * channels floats
 *                               (without the pair the backward needs none and looks at neither `workspace` argument).
 *   wcn_ln_act_fwd              writes y and stats [rows, 2] fp32 = (mean, rstd).
 *   wcn_ln_act_bwd              z is formed again in fp32 from x and stats (not read back from a rounded y), s = sigmoid(z):
 *                                   g  = dy * (act ? s (1 + z (1 - s)) : 1),   gw = g * weight
 *                                   dx = rstd (gw - mean_c(gw) - xhat mean_c(gw xhat))
 *                                   dweight = sum_rows g xhat,   dbias = sum_rows g      fp32 [channels], NULL without the pair
 *                               The column sums go through one partial slot per 64-row chunk in `workspace` and a fixed-order
 *                               second pass: no float atomics, no zero-filled workspace, two calls give bit-identical results.
 * The two skip paths, each the other's gradient (fp32 arithmetic, one rounding, no workspace; `h` may be NULL):
 *   wcn_channel_spread   out[n, c * r + j] = alpha * x[n, c] (+ h[n, c * r + j])        x [rows, cx]        -> out [rows, cx * r]
 *   wcn_channel_fold     out[n, c] = alpha * sum_{j < g} x[n, c * g + j] (+ h[n, c])    x [rows, cout * g]  -> out [rows, cout]
 * The decoder's skip is spread(x, h, r, 1) with the x-gradient fold(dout, NULL, r, 1); the encoder's is fold(x, h, g, 1 / g)
 * with spread(dout, NULL, g, 1 / g); dh is dout itself.  16-B accesses where the narrow side's channel count (cx / cout) is
 * a multiple of 8, r / g is 1, 2, 4 or 8 and the pointers are 16-B aligned; any channel count >= 1 and any r, g >= 1 go
 * through an element kernel.
 * Arguments are checked before any launch: a dtype or (LN) channel count outside the above, or a spread / fold row wider than
 * INT32_MAX channels -> WCN_ERROR_UNSUPPORTED_CONFIG; negative sizes (cx, cout, r, g < 1), rows > INT32_MAX, an `act` other
 * than 0 / 1, one of weight / bias without the other, a required pointer missing with rows > 0 (dweight / dbias / workspace are
 * required with the pair), a short workspace, a non-finite (or negative) eps, a non-finite alpha, LN buffers not 16-B aligned
 * -> WCN_ERROR_INVALID_PARAMETERS.  rows == 0 -> WCN_SUCCESS without a launch: nothing is written, a caller that wants zero
 * dweight / dbias fills them itself. */
int wcn_ln_act_supported(int32_t channels, int32_t dtype);
size_t wcn_ln_act_workspace_bytes(int64_t rows, int32_t channels);
int wcn_ln_act_fwd(const void* x, const float* weight, const float* bias, int64_t rows, int32_t channels, float eps,
                   int32_t act, int32_t dtype, void* y, float* stats, wcn_stream_t stream);
int wcn_ln_act_bwd(const void* dy, const void* x, const float* weight, const float* bias, const float* stats, int64_t rows,
                   int32_t channels, int32_t act, int32_t dtype, void* dx, float* dweight, float* dbias, void* workspace,
                   size_t workspace_bytes, wcn_stream_t stream);
int wcn_channel_spread(const void* x, const void* h, int64_t rows, int32_t cx, int32_t r, float alpha, int32_t dtype,
                       void* out, wcn_stream_t stream);
int wcn_channel_fold(const void* x, const void* h, int64_t rows, int32_t cout, int32_t g, float alpha, int32_t dtype,
                     void* out, wcn_stream_t stream);

/* ---- permuted rows: the attention sub-layer of a serialized-attention block (additions only, ABI unchanged) ----------------
 * x + drop_path(attn(norm1(x)[perm])[inverse_perm]) around the attention itself, as two row passes (csrc/ln_act.hip).  Rows
 * are [rows, channels] contiguous in `dtype`, widths and dtypes those of wcn_ln_act_supported; `index` / `inverse` are int64
 * [rows], a permutation of 0..rows-1 and its inverse.
 *   wcn_ln_permute_fwd   y[i] = LN(x[index[i]]) * weight + bias (the pair optional, fp32), the arithmetic of wcn_ln_act_fwd
 *                        with act = 0; stats [rows, 2] fp32 = (mean, rstd) of SOURCE row j = index[i].
 *   wcn_ln_permute_bwd   dy in output order: for every source row j, i = inverse[j], g = dy[i] * weight,
 *                        dx[j] = rstd (g - mean_c(g) - xhat mean_c(g xhat)), written once; dweight = sum_j dy[inverse[j]] xhat[j],
 *                        dbias = sum_j dy[inverse[j]] through the partial slots of wcn_ln_act_bwd (workspace of
 *                        wcn_ln_act_workspace_bytes; NULL / 0 without weight): no float atomics, bit-identical reruns.
 *   wcn_permute_add      out[t] = residual[t] + scale[s] * y[index[t]] with s = t, or s = index[t] when `scale_at_source`;
 *                        `residual` (rows of `dtype`) and `scale` (fp32 [rows]) may each be NULL.  Without scale: one fp32 add
 *                        per element, rounded once.  The gradient of y is the same call with the inverse index, no residual and
 *                        scale_at_source = 1; the gradient of residual is dout itself.
 * Every index is compared as unsigned with `rows` before it forms an address: an entry outside 0..rows-1 gives a row of zeros
 * (in wcn_ln_permute_bwd: dx[j] = 0 and no contribution to dweight / dbias; in the forward the stats of a source row that no
 * entry names stay unwritten) and never an out-of-bounds access.
 * Checks before any launch, as above: width / dtype -> WCN_ERROR_UNSUPPORTED_CONFIG; rows < 0 or > INT32_MAX, weight without
 * bias, a missing or misaligned pointer, a short workspace, a bad eps, scale_at_source other than 0 / 1 ->
 * WCN_ERROR_INVALID_PARAMETERS; rows == 0 -> WCN_SUCCESS without a launch. */
int wcn_ln_permute_fwd(const void* x, const int64_t* index, const float* weight, const float* bias, int64_t rows,
                       int32_t channels, float eps, int32_t dtype, void* y, float* stats, wcn_stream_t stream);
int wcn_ln_permute_bwd(const void* dy, const void* x, const int64_t* inverse, const float* weight, const float* stats,
                       int64_t rows, int32_t channels, int32_t dtype, void* dx, float* dweight, float* dbias, void* workspace,
                       size_t workspace_bytes, wcn_stream_t stream);
int wcn_permute_add(const void* y, const int64_t* index, const void* residual, const float* scale, int32_t scale_at_source,
                    int64_t rows, int32_t channels, int32_t dtype, void* out, wcn_stream_t stream);

/* ---- window grouping of voxels: a deterministic counting sort by 3-D window (ABI 11, additions only) ------------------------
 * The step that turns coordinates into the attention sequences of SpaceAttention (reference: voxel_encode(...,
 * encoding_method="counting_sort"), nn/functional/voxel_encode.py:237-316, on the two kernels of
 * csrc/window_grouping_kernels.cu: window_group_histogram_kernel :35-75 with find_batch_idx :14-25, and
 * window_group_scatter_kernel :82-99).
 * `coords` int32 [n, 3], `batch_offsets` int32 [num_batches + 1] (device; empty elements are legal).  `window`, `shift`
 * (= round(offset_fraction * window), voxel_encode.py:166-172), `min_coord` (column minimum over all rows) and `grid_shape`
 * (= ceil((max - min + shift + 1) / window), voxel_encode.py:249-255) are host values.  With W = prod(grid_shape) the
 * window code of voxel i of element b is
 *     w = (coords[i] + shift - min_coord) / window        per axis (operands non-negative: truncation = floor)
 *     code = b * W + (w.x * grid_shape.y + w.y) * grid_shape.z + w.z        int64
 * Outputs (device): `codes` int64 [n]; `perm` int64 [n] = the STABLE sort of the rows by code (inside a window rows appear
 * in ascending original index), `inverse_perm` int64 [n] with inverse_perm[perm[j]] = j; `cu_seqlens` int32 [S + 1] the
 * boundaries of the S non-empty windows in code order (cu_seqlens[S] = n) and `counts` int64 [S] their lengths, both
 * allocated by the caller for the worst case S = min(n, num_batches * W); `summary` int32 [2] = (S, max_count), the only
 * words the caller needs on the host.  S = -1: a voxel fell outside the announced box (min_coord / grid_shape do not fit the
 * coordinates, or batch_offsets does not cover n); nothing else is then meaningful.
 * The reference's scatter takes its slot with a racy atomic, so its row order inside a window changes from run to run.  Here
 * the slots are taken the same way (integer atomics only) and every window's segment is then sorted ascending - one wave
 * per segment of <= 64 rows, one workgroup per longer segment, in LDS - so two calls give bit-identical outputs.  Segments
 * longer than wcn_window_group_max_segment() = 8192 rows (32 KiB of LDS) are NOT sorted and their parts of perm /
 * inverse_perm are not written: the caller reads max_count from the summary and takes another path.  The prefix sum over the
 * dense histogram and the compaction of the non-empty bins are tile sums -> one-workgroup scan of the sums -> apply; no
 * kernel waits on another workgroup, every grid is capped at 4096 workgroups and strides.  The host is not read or waited
 * for by the call.
 *   wcn_window_group_max_segment     host-only: rows of the longest segment the call sorts (8192).
 *   wcn_window_group_workspace_bytes host-only: histogram (num_bins rounded up to 2048 int32), tile sums, n slot words.
 *   wcn_window_group                 the whole encode, seven launches on `stream`.
 * Arguments are checked before any launch: n < 0 or > INT32_MAX, num_batches < 1, a window or grid_shape entry < 1,
 * num_batches * W >= INT32_MAX - 2048, null pointers with n > 0 (summary and cu_seqlens always), a workspace that is short or
 * not 16-B aligned -> WCN_ERROR_INVALID_PARAMETERS.  n == 0 -> summary = (0, 0), cu_seqlens[0] = 0, no kernel launch. */
int32_t wcn_window_group_max_segment(void);
size_t wcn_window_group_workspace_bytes(int64_t n, int64_t num_bins);
int wcn_window_group(const int32_t* coords, int64_t n, const int32_t* batch_offsets, int32_t num_batches,
                     const int32_t window[3], const int32_t shift[3], const int32_t min_coord[3], const int32_t grid_shape[3],
                     int64_t* codes, int64_t* perm, int64_t* inverse_perm, int32_t* cu_seqlens, int64_t* counts,
                     int32_t* summary, void* workspace, size_t workspace_bytes, wcn_stream_t stream);

/* ---- points <-> voxels: the voxel map of a point cloud and the two feature kernels over it (ABI 12, additions only) ---------
 * Reference: point_pool / point_unpool (nn/functional/point_pool.py, point_unpool.py) on ToUnique (utils/unique.py:146-240):
 * torch.unique over rows, an argsort, a materialised features[perm] and torch_scatter.segment_csr.
 *   wcn_voxel_keys   `points` fp32 [n, 3], `batch_offsets` int32 [num_batches + 1] (device; empty elements are legal) ->
 *                    `keys` int64 [n] = b << 54 | (x + 2^17) << 36 | (y + 2^17) << 18 | (z + 2^17) with the cell
 *                    x = floor(p.x * inv_voxel_size) in fp32; the caller passes fp32(1.0 / voxel_size) with the quotient taken
 *                    in double, which is how the framework evaluates `points / voxel_size` for a host scalar on the device
 *                    (a true division puts points on a cell face elsewhere).  Biased 18-bit fields, so int64 order is the
 *                    lexicographic order of the signed (b, x, y, z) rows.  `status` int32 [1] is cleared by the call and receives bit 0:
 *                    a cell outside [-2^17, 2^17) (the key of that point is -1), bit 1: a row that belongs to no batch
 *                    element.  `points` == NULL: the keys are the caller's own codes, only the status is cleared.
 *   wcn_voxel_map    `sorted_keys` int64 [n] (ascending) and `perm` int64 [n] of a STABLE sort -> `unique_keys` int64 [M],
 *                    `unique_coords` int32 [M, 3] decoded from the keys (may be NULL), `csr_offsets` int64 [M + 1],
 *                    `to_orig` int64 [n] (voxel of every point), `to_unique` int64 [M] (first point of every voxel = its
 *                    smallest row), `batch_voxel_offsets` int32 [num_batches + 1] (voxels of the batch elements, from the
 *                    key's batch field; may be NULL), `summary` int32 [2] = (M, longest segment).  Every array is the
 *                    caller's, sized for M = n (csr_offsets n + 1); `perm` itself is the CSR's index list.  Tile sums ->
 *                    one-workgroup scan -> apply: no kernel waits on another workgroup.  The host is not read or waited for.
 *   wcn_csr_gather_reduce  out[s, :] = op over j in [offsets[s], offsets[s + 1]) of in[indices[j], :c], op 0 sum, 1 mean,
 *                    2 max, 3 min; `in` has `n_in` rows of stride `ld_in` >= c elements, `indices` int64 [nnz] (NULL = the
 *                    identity), `offsets` int64 [m + 1], `out` [m, c] and `in` of `dtype` (fp32 / fp16 / bf16), fp32
 *                    accumulation, one rounding.  Rows of a segment are added in ascending j; a segment longer than
 *                    wcn_csr_chunk_rows() = 256 rows is cut into chunks of that many rows, each added in ascending j into an
 *                    fp32 partial, and the partials are added in chunk order: a row's bits depend on its segment alone.  No
 *                    float atomics, no copy of in[indices].  max / min return the input element; `arg` int64 [m, c] (may
 *                    be NULL, max / min only) receives the FIRST extremum's row indices[j], -1 for an empty segment, whose
 *                    value is 0 (the wcn_segment_reduce convention).  `max_segment`: the longest segment if the caller
 *                    knows it (the chunk passes and the workspace are skipped when it is <= 256), -1 if not.  16-B or 8-B
 *                    pieces per lane when c, ld_in and both pointers allow, single elements otherwise; indices outside
 *                    [0, n_in) and offsets outside [0, nnz] contribute nothing.
 *   wcn_row_spread   out[i, :c] = scale(i) * src[to_orig[i], :], out[i, c:c + cs] = skip[i, :] (cs = 0: no second operand);
 *                    `out` has row stride `ld_out` >= c + cs, src is [m, c], skip [n, cs].  mode 0: scale = 1; 1: scale =
 *                    1 / (offsets[v + 1] - offsets[v]) for v = to_orig[i] (gradient of the mean); 2: out[i, ch] = src[v, ch]
 *                    if arg[v, ch] == i, else 0 (gradient of max / min).  Every element is written exactly once.
 * Arguments are checked before any launch: negative sizes, n / m / nnz > INT32_MAX, num_batches outside [1, 512] (0 allowed
 * for wcn_voxel_map without batch_voxel_offsets), an inv_voxel_size that is not positive and finite, an op / mode outside the lists,
 * ld_in < c, ld_out < c + cs, `arg` with sum / mean, a required pointer missing, sorted_keys or a workspace not 16-B aligned, a
 * short workspace -> WCN_ERROR_INVALID_PARAMETERS; an unknown dtype -> WCN_ERROR_UNSUPPORTED_CONFIG.  A call with no row
 * (n == 0, m == 0, c == 0) -> WCN_SUCCESS without a kernel launch (wcn_voxel_map still clears summary and the offsets). */
int32_t wcn_csr_chunk_rows(void);
int wcn_voxel_keys(const float* points, int64_t n, const int32_t* batch_offsets, int32_t num_batches, float inv_voxel_size,
                   int64_t* keys, int32_t* status, wcn_stream_t stream);
size_t wcn_voxel_map_workspace_bytes(int64_t n);
int wcn_voxel_map(const int64_t* sorted_keys, const int64_t* perm, int64_t n, int32_t num_batches, int64_t* unique_keys,
                  int32_t* unique_coords, int64_t* csr_offsets, int64_t* to_orig, int64_t* to_unique,
                  int32_t* batch_voxel_offsets, int32_t* summary, void* workspace, size_t workspace_bytes,
                  wcn_stream_t stream);
size_t wcn_csr_gather_reduce_workspace_bytes(int64_t nnz, int32_t c, int32_t op);
int wcn_csr_gather_reduce(const void* in, int64_t ld_in, int64_t n_in, const int64_t* indices, const int64_t* offsets,
                          int64_t m, int64_t nnz, int32_t c, int32_t dtype, int32_t op, int64_t max_segment, void* out,
                          int64_t* arg, void* workspace, size_t workspace_bytes, wcn_stream_t stream);
int wcn_row_spread(const void* src, const int64_t* to_orig, int64_t n, int64_t m, int32_t c, const void* skip, int32_t cs,
                   int64_t ld_out, int32_t mode, const int64_t* offsets, const int64_t* arg, int32_t dtype, void* out,
                   wcn_stream_t stream);

/* ---- lattice filters: permutohedral lattice and bilateral grid (ABI 13, additions only) -------------------------------------
 * Reference: nn/functional/permutohedral.py, nn/functional/bilateral_grid.py, geometry/coords/search/packed128_hashmap.py.
 * Keys are rows of key_dim <= 7 int32 coordinates, each in [-65536, 65535] (17-bit fields biased by 2^16, axis 0 in the most
 * significant field of a 128-bit number that travels as two 64-bit words hi, lo).
 *   wcn_hash128_insert  `table_keys` int64 [capacity, 2] (16-B aligned), `table_values` int32 [capacity], capacity a power of
 *                    two.  The call clears the values to -1 and inserts `coords` int32 [n, key_dim]: a slot is claimed under
 *                    linear probing by a 32-bit compare-and-swap on its value word (-1 -> row), the key words follow as one
 *                    plain 16-B store.  The caller guarantees DISTINCT keys; an inserting thread never compares keys.  `status`
 *                    int32 [1] is OR-ed with WCN_FLAG_COORD_RANGE (a coordinate outside the range, that row is not inserted)
 *                    and WCN_FLAG_TABLE_FULL; the caller clears it.  Searches belong in a later launch.
 *   wcn_hash128_search  out[j, i] = row of queries[i] + offsets[j] or -1 (absent, or outside the coordinate range); `queries`
 *                    int32 [m, key_dim], `offsets` int32 [k, key_dim] with 1 <= k <= 32 (NULL: k = 1, a zero offset), `out`
 *                    int32 [k, m].
 *   wcn_permuto_simplex `positions` fp32 [n, d], d <= 6, `scale` d HOST floats (the embedding's per-axis factors, formed by
 *                    the caller with the framework's own expression) -> per point the d + 1 vertices of the enclosing simplex:
 *                    entry e = i * (d + 1) + v gets `key_hi` / `key_lo` int64 (either may be NULL; the top bit of lo is flipped
 *                    so that a SIGNED 64-bit sort of lo, then of hi, orders the rows lexicographically), `keys` int32
 *                    [n (d + 1), d + 1] (may be NULL) and `bary` fp32 [n, d + 1].  fp32 arithmetic in the framework's order of
 *                    operations, never contracted into FMAs; rank ties go to the lower axis.
 *   wcn_grid_corners    the same for the 2^d corners of the enclosing grid cell: `floors` int64 [n, d] (may be NULL), keys as
 *                    above with entry e = i * 2^d + c, bit (d - 1 - j) of c stepping axis j, `weights` fp32 [n, 2^d] the
 *                    d-linear weights (product over the axes in ascending order).
 *                    Both OR WCN_FLAG_COORD_RANGE into `status` for a point with a key outside the range (NaN included).
 *   wcn_lattice_map     `sorted_hi` (NULL when key_dim * 17 <= 64), `sorted_lo` int64 [nnz] and `perm` int64 [nnz] of a STABLE
 *                    sort -> `unique_keys` int32 [V, key_dim] in lexicographic order, `inverse` int64 [nnz] (vertex of every
 *                    entry), `row_offsets` int64 [V + 1] (CSR by vertex over `perm`: inside a vertex the entries ascend),
 *                    `summary` int32 [2] = (V, longest row).  Arrays are the caller's, sized for V = nnz.
 *   wcn_lattice_plan    the rows of a CSR longer than wcn_lattice_chunk_rows() = 256 entries and their chunks, into `plan`
 *                    (wcn_lattice_plan_ints(nnz) int32 words); wcn_lattice_plan_items(nnz) = the partial rows a splat needs.
 *   Feature kernels, fp32, rows of `pitch` floats with pitch % 4 == 0 and 16-B aligned buffers (16-B pieces throughout):
 *   wcn_lattice_splat   out[r, :] = alpha * sum over j in [row_offsets[r], row_offsets[r + 1]) of w[e] * f[e / k, :] with
 *                    e = row_entries[j], ascending j, fp32 FMAs.  `plan` NULL: every row by one lane group.  Otherwise rows
 *                    longer than the chunk are cut into chunks, each summed the same way into `partials`
 *                    [wcn_lattice_plan_items(nnz), pitch], and added in chunk order.  No float atomics.
 *   wcn_lattice_blur    y[r] = s0 x[r] + s1 x[n1[r]] + s2 x[n2[r]]; n1, n2 int32 [v], -1 reads as zero, n2 may be NULL; x != y.
 *   wcn_lattice_slice   out[i] = alpha * sum over j < k of w[i, j] * x[idx[i, j]], ascending j; idx int64, -1 reads as zero.
 * Arguments are checked before any launch (WCN_ERROR_INVALID_PARAMETERS); an empty call returns WCN_SUCCESS without a launch.
 * Every grid is capped at 4096 workgroups and strides. */
int32_t wcn_lattice_chunk_rows(void);
int wcn_hash128_insert(int64_t* table_keys, int32_t* table_values, int64_t capacity, const int32_t* coords, int64_t n,
                       int32_t key_dim, int32_t* status, wcn_stream_t stream);
int wcn_hash128_search(const int64_t* table_keys, const int32_t* table_values, int64_t capacity, const int32_t* queries,
                       const int32_t* offsets, int64_t m, int32_t k, int32_t key_dim, int32_t* out, wcn_stream_t stream);
int wcn_permuto_simplex(const float* positions, int64_t n, int32_t d, const float* scale, int64_t* key_hi, int64_t* key_lo,
                        int32_t* keys, float* bary, int32_t* status, wcn_stream_t stream);
int wcn_grid_corners(const float* positions, int64_t n, int32_t d, int64_t* floors, int64_t* key_hi, int64_t* key_lo,
                     int32_t* keys, float* weights, int32_t* status, wcn_stream_t stream);
size_t wcn_lattice_map_workspace_bytes(int64_t nnz);
int wcn_lattice_map(const int64_t* sorted_hi, const int64_t* sorted_lo, const int64_t* perm, int64_t nnz, int32_t key_dim,
                    int32_t* unique_keys, int64_t* inverse, int64_t* row_offsets, int32_t* summary, void* workspace,
                    size_t workspace_bytes, wcn_stream_t stream);
int64_t wcn_lattice_plan_items(int64_t nnz);
int64_t wcn_lattice_plan_ints(int64_t nnz);
int wcn_lattice_plan(const int64_t* row_offsets, int64_t v, int64_t nnz, int32_t* plan, wcn_stream_t stream);
int wcn_lattice_splat(const float* f, const float* w, const int64_t* row_offsets, const int64_t* row_entries, int64_t v,
                      int64_t nnz, int32_t k, int32_t pitch, float alpha, const int32_t* plan, float* partials, float* out,
                      wcn_stream_t stream);
int wcn_lattice_blur(const float* x, const int32_t* n1, const int32_t* n2, float s0, float s1, float s2, int64_t v,
                     int32_t pitch, float* y, wcn_stream_t stream);
int wcn_lattice_slice(const float* x, const int64_t* idx, const float* w, int64_t n, int32_t k, int64_t v, int32_t pitch,
                      float alpha, float* out, wcn_stream_t stream);

/* ---- the fast bilateral solver and the kNN bilateral filter (ABI 14, additions only) -----------------------------------------
 * Reference: bilateral_solver of nn/functional/bilateral_grid.py and nn/functional/bilateral.py.  fp32 rows of `pitch` floats
 * as above; `neighbours` int32 [2 d, v] is the grid's table (rows 2a / 2a + 1 = one step forward / backward along axis a, -1
 * absent); the blur is the grid's: per axis y = b x + (c b) x[fwd], then y + a y[bwd], with the taps (a, b, c).
 *   wcn_lattice_max_grid  the cap of every grid of these kernels (4096) = the slots of one scalar's partials.
 *   wcn_lattice_row_grid  workgroups of a row kernel over `rows` rows of `pitch` floats = the partials it writes.
 *   wcn_bilateral_matvec  ap = (dc p) - lam n blur(n p) with per-vertex `nvec`, `dc` fp32 [v]; partials[g] = workgroup g's share
 *                    of sum p . ap in fp64.  `spare`: [2, v, pitch] floats.  2 d launches.
 *   wcn_bilateral_pcg     the preconditioned conjugate-gradient loop of the solver on the device.  In: `tbar` [v, pitch], `y` =
 *                    the start t / C, `minv` = 1 / diag(A).  `work` [6, v, pitch] floats (r, p, z, A p, two blur buffers),
 *                    `partials` fp64 [3, wcn_lattice_max_grid()], `state` fp64 [8] = (rz_old by iteration parity [2], |r0|,
 *                    done by parity [2], iterations carried out, a residual norm was not finite, 0).  max_iters iterations of
 *                    2 d + 2 launches each are enqueued; once |r| / |r0| < tol holds after the update of y and r, every later
 *                    launch that could write y, r, p or z returns at once, so y is the y of a loop that broke there.  Scalars:
 *                    fp64 products and sums, one partial per workgroup, partials added in index order; no float atomics.
 *   wcn_bilateral_knn_weights  weights[i, s] = w / max(sum over s of w, 1e-20), w = exp(-|src_xyz[nbr[i, s]] - query_xyz[i]|^2
 *                    / (2 sigma_xyz^2) - |src_feat[..] - query_feat[i]|^2 / (2 sigma_feat^2)); fp32 [*, dx] / [*, df] rows,
 *                    `nbr` int64 [m, k], the row sum in slot order; an index outside [0, n) weighs nothing. */
int32_t wcn_lattice_max_grid(void);
int32_t wcn_lattice_row_grid(int64_t rows, int32_t pitch);
int wcn_bilateral_matvec(const int32_t* neighbours, int32_t d, int64_t v, int32_t pitch, float tap_a, float tap_b, float tap_c,
                         const float* nvec, const float* dc, float lam, const float* p, float* spare, float* ap,
                         double* partials, wcn_stream_t stream);
int wcn_bilateral_pcg(const int32_t* neighbours, int32_t d, int64_t v, int32_t pitch, float tap_a, float tap_b, float tap_c,
                      const float* nvec, const float* dc, const float* minv, float lam, const float* tbar, float* y, float* work,
                      double* partials, double* state, int32_t max_iters, double tol, wcn_stream_t stream);
int wcn_bilateral_knn_weights(const float* src_xyz, const float* src_feat, const float* query_xyz, const float* query_feat,
                              const int64_t* nbr, int64_t n, int64_t m, int32_t k, int32_t dx, int32_t df, float sigma_xyz,
                              float sigma_feat, float* weights, wcn_stream_t stream);

/* ---- dense grids and point clouds: Grid / FactorGrid geometry (ABI 15, additions only) -------------------------------------
 * Reference: geometry/types/conversion/to_grid.py (points -> grid) and the F.grid_sample composition of
 * nn/modules/factor_grid.py / nn/functional/factor_grid.py (grid -> points, align_corners, border padding).
 *   wcn_grid_max_grid      the cap of every grid of these kernels (4096); they stride beyond it.
 *   wcn_grid_chunk_points  points of one chunk of a crowded cell in the backward (256).
 *   wcn_grid_point_keys    `points` fp32 [n, 3], `point_offsets` int64 [num_batches + 1] on the device, `dims` = vertices per
 *                    axis, `lo` / `scale` fp32 [3] on the host.  u_a = (p_a - lo_a) * scale_a clamped to [0, dims_a - 1] in
 *                    float (NaN -> 0).  WCN_GRID_KEY_CELL: keys[i] = b * cells + flat cell (int) u over `dims` (scale =
 *                    dims / (hi - lo)).  WCN_GRID_KEY_CORNER: i0_a = min(floor(u_a), max(dims_a - 2, 0)), fractions[i, a] =
 *                    u_a - i0_a, keys[i] = b * cells + flat base cell over max(dims_a - 1, 1) (scale = (dims - 1) / (hi - lo)).
 *   wcn_grid_sample        out[p, col0 + c] = sum over the 8 corners (dx, dy, dz; dz fastest) of w * grid[b, x, y, z, c], w =
 *                    wx * wy * wz in fp32, fp32 FMA accumulation, one rounding to `dtype`.  `strides` int64 [5] on the host:
 *                    the element strides of (b, x, y, z, c); `sorted_keys` / `perm`: the stable sort of the corner keys;
 *                    `fractions` in the points' own order; `out` rows of `out_pitch` elements.
 *   wcn_grid_sample_backward  d_grid through the same strides, every element written exactly once (0 where no point reaches
 *                    a vertex).  `cell_offsets` int64 [num_batches * cells + 1]: the rows of `sorted_keys` of every base cell.
 *                    `max_cell_points`: the longest cell if known, -1 if not; above wcn_grid_chunk_points() (or unknown) the
 *                    workspace of wcn_grid_sample_backward_workspace_bytes(n, channels) is needed.  No float atomics.
 * WCN_ERROR_INVALID_PARAMETERS: negative sizes, n or the vertex count above INT32_MAX, a missing pointer, a dims entry below
 * 1, col0 + channels beyond the pitch, a short workspace.  WCN_ERROR_UNSUPPORTED_CONFIG: an unknown dtype.  An empty call
 * returns success without a launch. */
enum wcn_grid_key_mode { WCN_GRID_KEY_CELL = 0, WCN_GRID_KEY_CORNER = 1 };
int32_t wcn_grid_max_grid(void);
int32_t wcn_grid_chunk_points(void);
int wcn_grid_point_keys(const float* points, int64_t n, const int64_t* point_offsets, int32_t num_batches, const int32_t* dims,
                        const float* lo, const float* scale, int32_t mode, int64_t* keys, float* fractions,
                        wcn_stream_t stream);
int wcn_grid_sample(const void* grid, const int64_t* strides, const int32_t* dims, int32_t channels, int32_t dtype,
                    int64_t num_batches, const int64_t* sorted_keys, const int64_t* perm, const float* fractions, int64_t n,
                    void* out, int64_t out_pitch, int64_t col0, wcn_stream_t stream);
size_t wcn_grid_sample_backward_workspace_bytes(int64_t n, int32_t channels);
int wcn_grid_sample_backward(const void* dy, int64_t dy_pitch, int64_t col0, const int64_t* strides, const int32_t* dims,
                             int32_t channels, int32_t dtype, int64_t num_batches, const int64_t* sorted_keys,
                             const int64_t* perm, const int64_t* cell_offsets, const float* fractions, int64_t n,
                             int64_t max_cell_points, void* d_grid, void* workspace, size_t workspace_bytes,
                             wcn_stream_t stream);

/* ---- segmented statistics and arithmetic on a ragged batch (ABI 16, additions only) ------------------------------------------
 * Reference: nn/functional/segmented_arithmetics.py, nn/functional/normalizations.py (segmented_norm / _layer_norm /
 * _range_norm) and global_scale of nn/functional/global_pool.py.  Rows are contiguous [rows, channels] in `dtype`, any
 * channels >= 1; `cu` int32 [num_segs + 1] on the device, segment b = rows [cu[b], cu[b + 1]), empty segments allowed, never
 * read on the host (spans are clamped to [0, rows]).  16-B pieces per lane where channels and every pointer allow, single
 * elements otherwise.  fp32 arithmetic, one rounding to `dtype`; no float atomics.  A segment is cut into chunks of
 * wcn_seg_chunk_rows() rows counted from its own first row, one workgroup per chunk, the chunks merged in chunk order by a
 * second launch: a segment's statistics depend bit for bit on that segment alone, and two calls agree bit for bit.
 *   wcn_seg_chunk_rows   rows of one chunk of a segment = rows of one tile of wcn_seg_apply (256).
 *   wcn_seg_max_grid     the cap of every grid of these kernels (4096); they stride beyond it.
 *   wcn_seg_stats_workspace_bytes  host-only: 256-B aligned int32 [num_segs + 1] plus (ceil(rows / chunk) + num_segs) chunk
 *                    slots of 2 (MOMENTS, DOT) or 4 (RANGE) fp32 [channels] planes.
 *   wcn_seg_stats    one read pass; writes the fp32 [num_segs, channels] planes out0 / out1.
 *                    WCN_SEG_MOMENTS (x): mean and the biased variance, centred (Welford / Chan merges), never E[x^2] - mean^2.
 *                    WCN_SEG_RANGE (x): min and max; arg0 / arg1 int64 [num_segs, channels] (each may be NULL) = the row of
 *                    the FIRST extremum.  An empty segment gives 0 and -1.  A NaN never compares and is passed over.
 *                    WCN_SEG_DOT (g, x, center): sum g and sum g (x - center[b]); `center` fp32 [num_segs, channels], NULL = 0;
 *                    with x NULL only out0 is written and out1 may be NULL.
 *                    Three launches (the chunk plan, the chunks, the merge).
 *   wcn_seg_apply    one streaming pass, out [rows, channels] in `dtype`:
 *                    WCN_SEG_ADD / SUB / MUL / DIV   out = x op y[b]; y [num_segs, channels] in `y_dtype` = `dtype` or
 *                    WCN_F32; DIV is a true division.
 *                    WCN_SEG_NORM       out = ((x - a[b]) r[b]) gamma + beta; a, r fp32 [num_segs, channels] (a NULL = 0),
 *                    gamma, beta fp32 [channels], each may be NULL.
 *                    WCN_SEG_NORM_BWD   out = r[b] (g gamma - s0[b] / n_b - xhat s1[b] / n_b), xhat = (x - a[b]) r[b], n_b the
 *                    segment's length, s0 / s1 the DOT planes of g gamma (center = a, then scaled by r).
 * WCN_ERROR_INVALID_PARAMETERS: an op / mode outside the lists, negative sizes, channels < 1, rows above INT32_MAX, a missing
 * required pointer, a misaligned pointer, a short or misaligned (16 B) workspace, a y_dtype that is neither `dtype` nor
 * WCN_F32.  WCN_ERROR_UNSUPPORTED_CONFIG: an unknown dtype.  Checked before any launch.  rows == 0 or num_segs == 0: success
 * without a launch; the statistics planes are zero-filled (arg planes -1). */
enum wcn_seg_mode { WCN_SEG_MOMENTS = 0, WCN_SEG_RANGE = 1, WCN_SEG_DOT = 2 };
enum wcn_seg_op { WCN_SEG_ADD = 0, WCN_SEG_SUB = 1, WCN_SEG_MUL = 2, WCN_SEG_DIV = 3, WCN_SEG_NORM = 4, WCN_SEG_NORM_BWD = 5 };
int32_t wcn_seg_chunk_rows(void);
int32_t wcn_seg_max_grid(void);
size_t wcn_seg_stats_workspace_bytes(int64_t rows, int64_t num_segs, int32_t channels, int32_t mode);
int wcn_seg_stats(int32_t mode, const void* x, const void* g, const float* center, const int32_t* cu, int64_t num_segs,
                  int64_t rows, int32_t channels, int32_t dtype, float* out0, float* out1, int64_t* arg0, int64_t* arg1,
                  void* workspace, size_t workspace_bytes, wcn_stream_t stream);
int wcn_seg_apply(int32_t op, const void* x, const void* g, const void* y, int32_t y_dtype, const float* a, const float* r,
                  const float* gamma, const float* beta, const float* s0, const float* s1, const int32_t* cu, int64_t num_segs,
                  int64_t rows, int32_t channels, int32_t dtype, void* out, wcn_stream_t stream);

/* ---- farthest point sampling on a ragged batch (ABI 17, additions only) -------------------------------------------------------
 * Reference: ops/sampling.py, csrc/farthest_point_sampling.cu.  `points` fp32 [n, 3] contiguous; `cu` int32 [total_segs + 1]
 * on the device, segment b = rows [cu[b], cu[b + 1]); `idx` int32 [total_segs, k] receives global rows.  A call serves the
 * num_segs segments named by `seg_ids` (int32 [num_segs] on the device; NULL = the segments 0 .. num_segs - 1) and writes
 * their rows of `idx` only; `max_len` is the caller's bound on their lengths, the only thing the host knows about them: it
 * picks the tier and the resident instantiation.  `start` int32 [total_segs] on the device holds the local row of sample 0
 * (NULL = 0).  Sample j > 0 is the row with the largest running distance min_s d(i, s) over the earlier samples, of equal
 * ones the lowest row; d = (dx dx + dy dy) + dz dz in fp32, every operation rounded once.  Once every row is taken the first
 * row repeats; an empty segment gets -1 in its k entries.  Both tiers give the same indices.
 *   WCN_FPS_RESIDENT  max_len <= wcn_fps_resident_max_points(): one workgroup of wcn_fps_block_threads() threads per segment,
 *                     points and distances in registers, all k samples in ONE launch; the grid is capped at
 *                     wcn_fps_max_grid() and strides over the segments.  No workspace.
 *   WCN_FPS_STREAMED  any length: wcn_fps_blocks_per_segment() workgroups per segment, k - 1 step launches and a last one,
 *                     enqueued back to back; running distances and per-workgroup partials live in the workspace
 *                     (wcn_fps_workspace_bytes, host-only; 16-B aligned).  A segment longer than blocks x threads strides.
 *   WCN_FPS_AUTO      resident where max_len allows, streamed otherwise.
 * cu, seg_ids and start are device data and are not trusted: a segment id outside [0, total_segs) is skipped, spans are
 * clamped to [0, n] (in the resident tier also to the instantiation's capacity), start to its segment.
 * WCN_ERROR_INVALID_PARAMETERS, before any launch: negative sizes, k < 1, n above INT32_MAX, an unknown tier, seg_ids NULL
 * with num_segs > total_segs, a missing or misaligned pointer, WCN_FPS_RESIDENT with max_len above the cap, a missing or short
 * workspace in the streamed tier.  num_segs == 0: success without a launch. */
enum wcn_fps_tier { WCN_FPS_AUTO = 0, WCN_FPS_RESIDENT = 1, WCN_FPS_STREAMED = 2 };
int64_t wcn_fps_resident_max_points(void);
int32_t wcn_fps_block_threads(void);
int32_t wcn_fps_blocks_per_segment(void);
int32_t wcn_fps_max_grid(void);
size_t wcn_fps_workspace_bytes(int64_t n, int64_t num_segs, int32_t k);
int wcn_fps(const float* points, const int32_t* cu, int64_t total_segs, const int32_t* seg_ids, int64_t num_segs, int64_t n,
            int32_t k, int64_t max_len, const int32_t* start, int32_t tier, void* workspace, size_t workspace_bytes,
            int32_t* idx, wcn_stream_t stream);

/* ---- axial rotary table and shared-tile attention kernels (ABI 18, additions only) ----------------------------------------------
 * wcn_rope_table_axes is wcn_rope_table with one frequency count per axis (the Volt volume transformer rotates 12 / 12 / 8
 * pairs by x / y / z): `freqs` is the concatenation float[counts[0] + counts[1] + counts[2]] on the device, `counts` a HOST
 * array; pair j of a token belongs to the axis a whose run holds j and turns by pos[a] * freqs[j], pos[a] =
 * float(coord[a]) - origin[a] + bias (fp32, one rounding per operation; a negative coordinate is a negative angle).  table
 * [total, sum(counts), 2] fp32 = (cos, sin); wcn_qk_prologue_fwd / _bwd consume it unchanged with rot_pairs = sum(counts).
 * 2 * sum(counts) > 256 -> WCN_ERROR_UNSUPPORTED_CONFIG; a negative count, counts NULL -> WCN_ERROR_INVALID_PARAMETERS.
 *
 * The attention kernels above are one wave per workgroup: every wave streams each 32-key (or 32-query) tile of its sequence
 * from global memory itself.  WCN_ATTN_SHARED runs the same products in workgroups of four waves: a work item is (sequence,
 * 128-row block, head), wave w owns rows 32 w .. 32 w + 31 of the block, and the workgroup stages every tile of the swept side
 * ONCE in LDS (row-major and as the transposed image the one-wave kernel builds), double-buffered, for all four waves.  Each
 * wave then issues exactly the one-wave kernel's sequence - same tile order, same MFMA chains, same exp2-domain softmax, same
 * stores - so out, lse, dq, dk, dv carry the same bits under either variant, and everything said above holds for both: empty
 * sides, rows outside every sequence not written, fixed-order sums, q_splits (partials in the same layout), the host never reads
 * cu_*.
 *   wcn_attn_varlen_variant   host-only: the variant WCN_ATTN_AUTO resolves to for `direction` (0 = forward, 1 = backward), a
 *                             pure function of these numbers: WCN_ATTN_SHARED when the longest swept side (max_seqlen_k
 *                             forward; max(max_seqlen_q, max_seqlen_k) backward, whose dQ kernel sweeps the keys and whose
 *                             dK/dV kernel the queries) is at least 512 rows, WCN_ATTN_ONE_WAVE otherwise (and for an empty
 *                             call).  Measured: docs/OPTIMISATION_LOG.md section AG.
 *   wcn_attn_varlen_kv_fwd_v / wcn_attn_varlen_kv_bwd_v   the entry points above with `variant` (an unknown value ->
 *                             WCN_ERROR_INVALID_PARAMETERS).  The entry points without it, packed and separate, call
 *                             WCN_ATTN_AUTO. */
enum wcn_attn_variant { WCN_ATTN_AUTO = 0, WCN_ATTN_ONE_WAVE = 1, WCN_ATTN_SHARED = 2 };
int wcn_rope_table_axes(const void* coords, int32_t coords_float, int64_t total, const float* origin, float bias,
                        const float* freqs, const int32_t counts[3], float* table, wcn_stream_t stream);
int32_t wcn_attn_varlen_variant(int64_t num_seqs, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t heads, int32_t direction);
int wcn_attn_varlen_kv_fwd_v(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                             const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs, int64_t total_q, int64_t total_k,
                             int32_t heads, int32_t head_dim, int32_t max_seqlen_q, int32_t max_seqlen_k, float softmax_scale,
                             int32_t dtype, void* out, float* lse, int32_t variant, wcn_stream_t stream);
int wcn_attn_varlen_kv_bwd_v(const void* dout, const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                             const void* out, const float* lse, const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs,
                             int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim, int32_t max_seqlen_q,
                             int32_t max_seqlen_k, float softmax_scale, int32_t dtype, void* dq, int64_t dq_stride, void* dk,
                             void* dv, int64_t dkv_stride, int32_t q_splits, void* workspace, size_t workspace_bytes,
                             int32_t variant, wcn_stream_t stream);

/* ---- flexible-dual-grid mesh extraction (additions only; wcn_abi_version() stays 18, which tests/test_volt_api.py pins) --------
 * Definition: DESIGN.md 4.28. Every voxel row carries three flags (`flags` uint8 [n, 3], non-zero = set): flag a says the
 * surface crosses the primal edge along axis a through the voxel's maximum corner.  A flagged edge whose four surrounding
 * voxels q0 .. q3 all exist yields quad (q0, q1, q2, q3) and two faces; the others are dropped.  The voxels come from `nbr`
 * int32 [n, pitch], the kernel map of the voxel set onto itself with kernel_size (2, 2, 2) (column 4 i + 2 j + l = the row
 * at +(i, j, l) or -1; pitch = wcn_kmap_row_pitch(8) = 8, 16-B aligned); an entry outside [0, n) counts as absent.  Quads are
 * ordered by (row, axis), quad i owns faces 2 i and 2 i + 1; indices are local to the scene: row - offsets[b], b = column 0 of
 * `coords` int32 [n, 4], `offsets` int32 [num_batches + 1] on the device.
 *   wcn_fdg_supported  host-only: 1 if dual_dtype is f32 / f16 / bf16 and lerp_dtype is one of them or negative (no weights).
 *   wcn_fdg_workspace  bytes of the workspace both calls share (16-B aligned), host-only.
 *   wcn_fdg_count      kept (row, axis) pairs per row and 256-row tile into the workspace, then quad_offsets [num_batches + 1]:
 *                      quads in front of every scene, the last entry the total.  n == 0 writes zeros.
 *   wcn_fdg_emit       from the workspace a wcn_fdg_count call on the same nbr / flags left: verts fp32 [n, 3] =
 *                      ((float(coord) + dual) * voxel_size) + lo, three fp32 operations each rounded once (`dual` [n, 3] in
 *                      dual_dtype, widened first); quads int32 [capacity, 4]; faces int32 [2 capacity, 3].  Each of the three
 *                      may be NULL (skipped); nothing is written for a quad at or beyond `capacity`.  Split of quad i: with
 *                      `lerp` ([n, 1] in lerp_dtype, widened) faces (q0,q1,q2),(q0,q2,q3) iff w0 w2 > w1 w3, else
 *                      (q0,q1,q3),(q3,q1,q2); without, the same choice iff |n(q0,q1,q2).n(q0,q2,q3)| > |n(q0,q1,q3).n(q3,q1,q2)|
 *                      on the vertices above, n(a,b,c) = cross(b - a, c - a), every fp32 operation rounded once (DESIGN.md
 *                      4.28 lists them).  No atomics: the output does not depend on the launch.
 * WCN_ERROR_INVALID_PARAMETERS, before any launch: negative sizes, n >= 2^31 / 6, pitch != 8, a missing or misaligned pointer,
 * a short workspace, verts without dual, faces without dual and lerp.  WCN_ERROR_UNSUPPORTED_CONFIG: an unknown dtype. */
int wcn_fdg_supported(int32_t dual_dtype, int32_t lerp_dtype);
size_t wcn_fdg_workspace(int64_t n);
int wcn_fdg_count(const int32_t* nbr, int32_t pitch, const uint8_t* flags, int64_t n, const int32_t* offsets,
                  int32_t num_batches, void* workspace, size_t workspace_bytes, int32_t* quad_offsets, wcn_stream_t stream);
int wcn_fdg_emit(const int32_t* nbr, int32_t pitch, const uint8_t* flags, const int32_t* coords, int64_t n,
                 const int32_t* offsets, int32_t num_batches, const void* dual, int32_t dual_dtype, const void* lerp,
                 int32_t lerp_dtype, float voxel_size, const float lo[3], const void* workspace, size_t workspace_bytes,
                 int64_t capacity, float* verts, int32_t* quads, int32_t* faces, wcn_stream_t stream);

/* ---- ragged row repack: cat <-> pad <-> patch (csrc/pad.hip; additions only, wcn_abi_version() stays 18) -------------------
 * A batch of num_segs segments, segment b of cu[b + 1] - cu[b] rows (`cu` int32 [num_segs + 1] on the device, never read on
 * the host).  A layout says where a segment's first row is: `starts` int32 [num_segs + 1] on the device (cat: cu itself;
 * patch: the patch offsets), or NULL with `pitch` = M for the padded [num_segs, M, c] tensor (rows must equal num_segs *
 * pitch).  Rows are `row_bytes` bytes of elements of `elem_bytes` (1, 2, 4 or 8) bytes: a byte copy, any dtype.
 *   wcn_pad_repack   every destination row is written exactly once: row j of its segment gets the segment's source row j if
 *                    j < len_b, else the fill element (the low elem_bytes bytes of `fill_bits`) in every element; so do rows
 *                    past the last segment and rows whose source row lies outside [0, src_rows).  src NULL = fill only: rows
 *                    with j < len_b are left as they are (clear_padding).  One launch, no atomics, no prior zero fill;
 *                    16-B pieces where row_bytes and both pointers allow, else 8, 4, 2 or 1 (never below elem_bytes).
 *   wcn_pad_max_grid / wcn_pad_block_threads   the grid cap (the kernel strides beyond it) and the threads of a workgroup;
 *                    a thread moves one piece.
 * WCN_ERROR_INVALID_PARAMETERS, before any launch: negative sizes, sizes above INT32_MAX, row_bytes not a multiple of
 * elem_bytes, a pitch layout whose rows are not num_segs * pitch, a missing or misaligned pointer, rows without a segment.
 * WCN_ERROR_UNSUPPORTED_CONFIG: another elem_bytes.  dst_rows == 0: success without a launch. */
int32_t wcn_pad_max_grid(void);
int32_t wcn_pad_block_threads(void);
int wcn_pad_repack(const void* src, void* dst, const int32_t* cu, int64_t num_segs, const int32_t* src_starts,
                   int64_t src_pitch, int64_t src_rows, const int32_t* dst_starts, int64_t dst_pitch, int64_t dst_rows,
                   int64_t row_bytes, int32_t elem_bytes, uint64_t fill_bits, wcn_stream_t stream);

/* ---- per-segment GEMM over contiguous rows (csrc/seg_bmm.hip; additions only) --------------------------------------------------
 * x [rows, .] in `dtype` (f32 / f16 / bf16), W [num_segs, cin, cout] in the same dtype, `cu` as above.  fp32 accumulation, one
 * rounding; fp32 operands stay fp32 (v_mfma_f32_16x16x4_f32), the half types use v_mfma_f32_16x16x32.  1 <= cin, cout <=
 * wcn_seg_bmm_max_channels() (256).  No float atomics; no host read; two calls agree bit for bit.
 *   wcn_seg_bmm        transpose_w == 0: y [rows, cout] = x [rows, cin] @ W[seg(r)]; else y [rows, cin] = x [rows, cout] @
 *                      W[seg(r)]^T (the data gradient).  A row's result depends bit for bit on that row and its weight alone.
 *                      Two launches (the tile plan, the tiles of wcn_seg_bmm_tile_rows() rows).
 *   wcn_seg_bmm_wgrad  dw [num_segs, cin, cout] in `dtype` = X_b^T dY_b: chunks of wcn_seg_bmm_chunk_rows() rows counted from
 *                      the segment's own first row, fp32 partial sums added in chunk order, rounded once.  dw[b] depends bit for
 *                      bit on segment b alone; a segment without rows gives exact zeros.  Three launches.
 *   wcn_seg_bmm_workspace_bytes  host-only; wgrad != 0 for wcn_seg_bmm_wgrad.  16-B aligned workspace.
 * WCN_ERROR_INVALID_PARAMETERS: negative sizes, channels < 1, rows above INT32_MAX, num_segs above 65535, a missing or
 * misaligned pointer, a short workspace.  WCN_ERROR_UNSUPPORTED_CONFIG: an unknown dtype, channels above the cap.  Checked
 * before any launch.  rows == 0 or num_segs == 0: success without a launch (dw zero-filled). */
int32_t wcn_seg_bmm_max_channels(void);
int32_t wcn_seg_bmm_tile_rows(void);
int32_t wcn_seg_bmm_chunk_rows(void);
size_t wcn_seg_bmm_workspace_bytes(int64_t rows, int64_t num_segs, int32_t cin, int32_t cout, int32_t wgrad);
int wcn_seg_bmm(const void* x, const void* w, const int32_t* cu, int64_t num_segs, int64_t rows, int32_t cin, int32_t cout,
                int32_t transpose_w, int32_t dtype, void* y, void* workspace, size_t workspace_bytes, wcn_stream_t stream);
int wcn_seg_bmm_wgrad(const void* x, const void* dy, const int32_t* cu, int64_t num_segs, int64_t rows, int32_t cin,
                      int32_t cout, int32_t dtype, void* dw, void* workspace, size_t workspace_bytes, wcn_stream_t stream);

/* ---- EdgeConv without an edge tensor (csrc/edgeconv.hip; additions only, wcn_abi_version() stays 18) -------------------------
 * out[i] = max over the list of i of leaky_relu(a z_e + s), z[e = (i <- j)] = P[j] + Q[i]: the edge pre-activation of
 * Linear(cat(x_j, x_i)) split into the per-point products P [num_inputs, channels] (row pitch ld_p floats) and Q
 * [num_queries, channels] (row pitch ld_q), which the caller makes with a library GEMM.  fp32; 1 <= channels <=
 * wcn_edgeconv_max_channels() (512), 16-B pieces when channels % 4 == 0 and the pitches and pointers allow, else single
 * channels.  Lists: nbr int32 [num_edges] rows of P, and either row_splits int64 [num_queries + 1] (ragged, empty lists
 * allowed) or NULL with the uniform length k (k * num_queries == num_edges).  Everything on the device, nothing read on the
 * host; spans are clamped to the edges there are and a neighbour outside [0, num_inputs) is skipped.  No float atomics: every
 * sum has a fixed order and two calls agree bit for bit.  a, s [channels]: gamma * rstd and beta - a * mean (training: batch
 * statistics, eval: running ones, no BatchNorm: 1 and 0).
 *   wcn_edgeconv_stats           mean / biased variance [channels] of z over all edges, one pass: sums of (z - p) and (z - p)^2
 *                                around the pivot p = P[nbr[0]] + Q[0], wcn_edgeconv_sum_blocks() workgroup partials merged in
 *                                fp64 in workgroup order.  The count is num_edges.
 *   wcn_edgeconv_forward         out [num_queries, channels] and, if arg != NULL, the slot (position in its list) of the FIRST
 *                                maximum as arg_bytes-wide integers (1, 2 or 4; wcn_edgeconv_arg_bytes(longest list) is the
 *                                narrowest that holds it).  An empty list: out = 0, arg = -1.
 *   wcn_edgeconv_backward_sums   dbeta = sum g, dgamma = sum g (z - mu) rstd over the arg-max entries, g = grad_out * (u > 0 ? 1 :
 *                                slope); mu / rstd NULL = 0 / 1.
 *   wcn_edgeconv_backward_query  dq[i] (pitch ld_q) = sum over the list of i, in list order, of dz_e = a (t_e - k0 - zhat_e k1),
 *                                t_e = g at the arg-max edge and 0 elsewhere.  k0 = dbeta / E and k1 = dgamma / E (training) or
 *                                both NULL (eval, no BatchNorm: dz_e = a t_e).
 *   wcn_edgeconv_backward_input  dp[j] (pitch ld_p) = the same dz_e summed over the incoming edges of j in incoming order: perm
 *                                int32 [num_edges] = the edges sorted by neighbour, ties ascending; offsets int64 [num_inputs +
 *                                1]; edge_query int32 [num_edges] the query of every edge (ragged lists; uniform: e / k).  A row
 *                                of more than wcn_csr_chunk_rows() incoming edges is cut into chunks added in chunk order.
 * WCN_ERROR_INVALID_PARAMETERS, before any launch: negative sizes, sizes above INT32_MAX, a pitch below channels, k * num_queries
 * != num_edges, a missing or misaligned pointer (arg and the input workspace: 16 B / 256 B), another arg_bytes, a short
 * workspace, statistics of no edge.  WCN_ERROR_UNSUPPORTED_CONFIG: channels above the cap. */
int32_t wcn_edgeconv_max_channels(void);
int32_t wcn_edgeconv_sum_blocks(void);
int32_t wcn_edgeconv_arg_bytes(int64_t longest_list);
size_t wcn_edgeconv_sums_workspace_bytes(int32_t channels);
size_t wcn_edgeconv_backward_input_workspace_bytes(int64_t num_edges, int32_t channels);
int wcn_edgeconv_stats(const float* P, int64_t ld_p, const float* Q, int64_t ld_q, const int32_t* nbr, const int64_t* row_splits,
                       int32_t k, int64_t num_edges, int64_t num_queries, int64_t num_inputs, int32_t channels, float* mean,
                       float* var, void* workspace, size_t workspace_bytes, wcn_stream_t stream);
int wcn_edgeconv_forward(const float* P, int64_t ld_p, const float* Q, int64_t ld_q, const int32_t* nbr, const int64_t* row_splits,
                         int32_t k, int64_t num_edges, int64_t num_queries, int64_t num_inputs, int32_t channels, const float* a,
                         const float* s, float slope, float* out, void* arg, int32_t arg_bytes, wcn_stream_t stream);
int wcn_edgeconv_backward_sums(const float* P, int64_t ld_p, const float* Q, int64_t ld_q, const int32_t* nbr,
                               const int64_t* row_splits, int32_t k, int64_t num_edges, int64_t num_queries, int64_t num_inputs,
                               int32_t channels, const float* a, const float* s, const float* mu, const float* rstd, float slope,
                               const float* grad_out, const void* arg, int32_t arg_bytes, float* dbeta, float* dgamma,
                               void* workspace, size_t workspace_bytes, wcn_stream_t stream);
int wcn_edgeconv_backward_query(const float* P, int64_t ld_p, const float* Q, int64_t ld_q, const int32_t* nbr,
                                const int64_t* row_splits, int32_t k, int64_t num_edges, int64_t num_queries, int64_t num_inputs,
                                int32_t channels, const float* a, const float* s, const float* mu, const float* rstd,
                                const float* k0, const float* k1, float slope, const float* grad_out, const void* arg,
                                int32_t arg_bytes, float* dq, wcn_stream_t stream);
int wcn_edgeconv_backward_input(const float* P, int64_t ld_p, const float* Q, int64_t ld_q, const int32_t* nbr,
                                const int64_t* row_splits, int32_t k, int64_t num_edges, int64_t num_queries, int64_t num_inputs,
                                int32_t channels, const int32_t* perm, const int64_t* offsets, const int32_t* edge_query,
                                const float* a, const float* s, const float* mu, const float* rstd, const float* k0,
                                const float* k1, float slope, const float* grad_out, const void* arg, int32_t arg_bytes, float* dp,
                                void* workspace, size_t workspace_bytes, wcn_stream_t stream);

/* ---- split-key attention: few queries against a long context (additions only; wcn_abi_version() stays 18) -----------------------
 * The forward and the dQ kernel give one wave or workgroup per (sequence, query block, head), which sweeps every key of the
 * sequence serially; a few learned queries per scene against 10^4 .. 10^5 points (MaskFormer's decoder) then launch a handful
 * of work items that each walk thousands of key tiles.  With k_splits = S > 1 a work item is (sequence, query block, split,
 * head): with nb = ceil(len_k / 32) and per = ceil(nb / S), split j sweeps the 32-key blocks [j per, min((j + 1) per, nb)) of
 * its sequence (read from cu_k on the device; trailing shares may be empty; the same shares under both variants) and writes
 * fp32 partials to the workspace:
 *   forward  o [S, total_q, heads, head_dim] the unnormalised accumulator, then ml [S, total_q, heads, 2] the share's running
 *            maximum (exp2 domain) and sum; an empty share writes (-inf, 0) and o = 0.  A combine kernel forms, per (query,
 *            head) and with j = 0 .. S - 1 in that order, M = max_j m_j, L = sum_j exp2(m_j - M) l_j,
 *            out = sum_j exp2(m_j - M) o_j / L, lse = (M + log2 L) ln 2; no key at all: out = 0, lse = -inf.
 *   dQ       dq_j [S, total_q, heads, head_dim] unscaled (P comes from the final lse: nothing to renormalise); a reduce kernel
 *            adds them in the order 0 .. S - 1, scales, casts, stores.  dK/dV keeps its q_splits and is otherwise unchanged.
 * Every partial a later kernel reads is written first, so the workspace's previous contents never matter; no float atomics;
 * one-wave and shared give the same bits for every S; S = 1 launches the unsplit kernels (the bits of the entry points above).
 *   wcn_attn_varlen_k_splits                host-only: the count the library chooses for k_splits = 0 (direction 0 = forward,
 *                                           1 = backward; one rule for both).  1 when the unsplit launch already has 4096
 *                                           work items, counted in 128-query blocks: num_seqs * ceil(max_seqlen_q / 128) *
 *                                           heads; otherwise enough splits to reach 4096, at most ceil(max_seqlen_k / 32) / 17
 *                                           (a split sweeps at least 17 key blocks), at most what keeps the partials of
 *                                           num_seqs * max_seqlen_q rows at head_dim 64 under 256 MiB, at most 64.  Non-
 *                                           increasing in num_seqs and max_seqlen_q.  The count is in 128-query blocks whatever
 *                                           variant the call names (a sweep long enough to split is one WCN_ATTN_AUTO gives to the
 *                                           shared kernels): a forced WCN_ATTN_ONE_WAVE launches four times the work items the
 *                                           target means, which costs nothing but is not what was measured.  `direction` is
 *                                           accepted and ignored.  Constants: docs/OPTIMISATION_LOG.md section AN.
 *   wcn_attn_varlen_ksplit_workspace_bytes  host-only: direction 0: k_splits > 1 ? 4 k_splits total_q heads (head_dim + 2) : 0;
 *                                           direction 1: wcn_attn_varlen_kv_workspace_bytes(.., q_splits) plus, when
 *                                           k_splits > 1, 4 k_splits total_q heads head_dim (k_splits as resolved, not 0).
 *   wcn_attn_varlen_kv_fwd_s / _kv_bwd_s    the _v entry points with k_splits (0: the rule, 1: no split, < 0 ->
 *                                           WCN_ERROR_INVALID_PARAMETERS) and, for the forward, a workspace.  A needed workspace
 *                                           that is NULL, not 16-byte aligned or smaller than the function above reports ->
 *                                           WCN_ERROR_INVALID_PARAMETERS, nothing launched.  Every other entry point stays at
 *                                           one split. */
int32_t wcn_attn_varlen_k_splits(int64_t num_seqs, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t heads, int32_t direction);
size_t wcn_attn_varlen_ksplit_workspace_bytes(int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim,
                                              int32_t q_splits, int32_t k_splits, int32_t direction);
int wcn_attn_varlen_kv_fwd_s(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                             const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs, int64_t total_q, int64_t total_k,
                             int32_t heads, int32_t head_dim, int32_t max_seqlen_q, int32_t max_seqlen_k, float softmax_scale,
                             int32_t dtype, void* out, float* lse, int32_t variant, int32_t k_splits, void* workspace,
                             size_t workspace_bytes, wcn_stream_t stream);
int wcn_attn_varlen_kv_bwd_s(const void* dout, const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                             const void* out, const float* lse, const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs,
                             int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim, int32_t max_seqlen_q,
                             int32_t max_seqlen_k, float softmax_scale, int32_t dtype, void* dq, int64_t dq_stride, void* dk,
                             void* dv, int64_t dkv_stride, int32_t q_splits, int32_t k_splits, void* workspace,
                             size_t workspace_bytes, int32_t variant, wcn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* WCN_H_ */
