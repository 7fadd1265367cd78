// resample.hip - data movement of the sparse resampling layer (space-to-channel, channel-to-space, subdivide, up/down-sample,
// prune) over a CHILD TABLE: tbl[p * pitch + col] = fine row that is one of the f^3 children of coarse row p, or -1.
//
//   wcn_resample_pack     dst[p][s*C .. (s+1)*C) = src[tbl[p][col(s)]] or 0      one pass over the packed tensor [P, n_per*C]:
//                         the zeros of absent children are written by the same store stream, no memset + scatter
//   wcn_resample_unpack   dst[tbl[p][col(s)]] = src[p][s*C .. (s+1)*C)           (broadcast: src[p][0 .. C) for every slot)
//   wcn_resample_expand   children of the parents a mask keeps: count -> exclusive scan -> emit (coordinates, child table,
//                         batch offsets); with n_per = 1 the compaction behind prune
//
// Channel slot s = (x mod f) + f (y mod f) + f^2 (z mod f) is the reference's numbering (nn/modules/sparse_resample.py:202-203);
// the tables of wcn_cells_stride_emit and of a kernel map with kernel_size == stride == f enumerate the window with z fastest
// (col = (x f + y) f + z), the tables of wcn_resample_expand with col = s: `slot_order` names which one a table uses.
//
// pack / unpack are pure copies, bound by HBM: a workgroup owns a group of consecutive coarse rows (about 32 KB of packed
// row), a lane moves one 16-B piece (or one element when C * sizeof(T) is not a multiple of 16), adjacent lanes hold adjacent
// pieces of one child row, so every access is a whole-row segment and the table word of a (row, slot) is one address for
// all lanes that share it.  No LDS, no atomics; the results do not depend on the launch shape.
// Reference (pure torch): zeros + indexed write / indexed read, unique, repeat_interleave, nonzero
// (warpconvnet/nn/modules/sparse_resample.py:155-287, nn/functional/sparse_ops.py:33-65).

#include "wcn_common.h"

namespace wcn {

constexpr int kRsMaxPer = 64;      // f <= 4
constexpr int kRsThreads = 256;
constexpr int kRsUnitsPerWg = 2048;  // 32 KB of 16-B pieces per workgroup
constexpr int kRsMaskU8 = 3;       // mask_dtype of wcn_resample_expand: bytes (a torch bool); 0 / 1 / 2 = wcn_dtype

struct SlotCols {
  int8_t col[kRsMaxPer];  // table column of channel slot s
};

static inline bool slot_cols(int n_per, int factor, int slot_order, SlotCols* sc) {
  if (factor < 1 || factor > 4 || n_per != factor * factor * factor) return false;
  if (slot_order != WCN_SLOT_X_FASTEST && slot_order != WCN_SLOT_Z_FASTEST) return false;
  for (int s = 0; s < n_per; ++s) {
    const int x = s % factor, y = (s / factor) % factor, z = s / (factor * factor);
    sc->col[s] = (int8_t)(slot_order == WCN_SLOT_Z_FASTEST ? (x * factor + y) * factor + z : s);
  }
  return true;
}

template <typename U> __device__ __forceinline__ U zero_unit();
template <> __device__ __forceinline__ uint4 zero_unit<uint4>() { return make_uint4(0u, 0u, 0u, 0u); }
template <> __device__ __forceinline__ uint32_t zero_unit<uint32_t>() { return 0u; }
template <> __device__ __forceinline__ uint16_t zero_unit<uint16_t>() { return (uint16_t)0; }

// u = units (16-B pieces or elements) per child row; rows = coarse rows per workgroup
template <typename U>
__global__ __launch_bounds__(kRsThreads) void resample_pack_kernel(const U* __restrict__ src, const int32_t* __restrict__ tbl,
                                                                   int64_t n_src, int64_t n_parent, int n_per, int pitch,
                                                                   SlotCols sc, int u, int rows, U* __restrict__ dst) {
  const int64_t p0 = (int64_t)blockIdx.x * rows;
  const int todo = (int)min((int64_t)rows, n_parent - p0) * n_per * u;
  for (int i = threadIdx.x; i < todo; i += kRsThreads) {
    const int q = i / u, v = i - q * u;           // (row, slot) of the group, piece of the child row
    const int pl = q / n_per, s = q - pl * n_per;
    const int32_t r = tbl[(p0 + pl) * pitch + sc.col[s]];
    U val = zero_unit<U>();
    if (r >= 0 && r < n_src) val = src[(int64_t)r * u + v];
    dst[(p0 * n_per) * u + i] = val;
  }
}

template <typename U>
__global__ __launch_bounds__(kRsThreads) void resample_unpack_kernel(const U* __restrict__ src, const int32_t* __restrict__ tbl,
                                                                     int64_t n_parent, int64_t n_dst, int n_per, int pitch,
                                                                     SlotCols sc, int u, int rows, int broadcast,
                                                                     U* __restrict__ dst) {
  const int64_t p0 = (int64_t)blockIdx.x * rows;
  const int todo = (int)min((int64_t)rows, n_parent - p0) * n_per * u;
  for (int i = threadIdx.x; i < todo; i += kRsThreads) {
    const int q = i / u, v = i - q * u;
    const int pl = q / n_per, s = q - pl * n_per;
    // no table: the dense subdivision, child (p, s) is row p * n_per + s
    const int64_t r = tbl ? (int64_t)tbl[(p0 + pl) * pitch + sc.col[s]] : (p0 + pl) * n_per + s;
    if (r < 0 || r >= n_dst) continue;
    const U val = broadcast ? src[(p0 + pl) * u + v] : src[(p0 * n_per) * u + i];
    dst[r * u + v] = val;
  }
}

template <typename U>
static int pack_u(const void* src, const int32_t* tbl, int64_t n_src, int64_t P, int n_per, int pitch, const SlotCols& sc, int u,
                  void* dst, hipStream_t s) {
  const int rows = max(1, kRsUnitsPerWg / (n_per * u));
  hipLaunchKernelGGL((resample_pack_kernel<U>), dim3((unsigned)ceil_div(P, rows)), dim3(kRsThreads), 0, s, (const U*)src, tbl,
                     n_src, P, n_per, pitch, sc, u, rows, (U*)dst);
  return launch_status();
}

template <typename U>
static int unpack_u(const void* src, const int32_t* tbl, int64_t P, int64_t n_dst, int n_per, int pitch, const SlotCols& sc,
                    int u, int broadcast, void* dst, hipStream_t s) {
  const int rows = max(1, kRsUnitsPerWg / (n_per * u));
  hipLaunchKernelGGL((resample_unpack_kernel<U>), dim3((unsigned)ceil_div(P, rows)), dim3(kRsThreads), 0, s, (const U*)src, tbl,
                     P, n_dst, n_per, pitch, sc, u, rows, broadcast, (U*)dst);
  return launch_status();
}

// ---- expand --------------------------------------------------------------------------------------------------------------
struct ExpandWs {
  int32_t* cnt;   // [P]      kept children per parent
  int32_t* tile;  // [T + 1]  kept children in front of every 256-row tile, the last entry their total
};
static inline int64_t expand_tiles(int64_t P) { return ceil_div(P > 0 ? P : 0, kRsThreads); }
static inline ExpandWs carve_expand(void* ws, int64_t P) {
  ExpandWs w;
  w.cnt = (int32_t*)ws;
  w.tile = w.cnt + ((P + 3) & ~(int64_t)3);
  return w;
}

__device__ __forceinline__ bool mask_keeps(const void* mask, int mask_dtype, int64_t at) {
  if (!mask) return true;
  switch (mask_dtype) {
    case WCN_F32: return ((const float*)mask)[at] != 0.0f;
    case WCN_F16:
    case WCN_BF16: return (((const uint16_t*)mask)[at] & 0x7FFFu) != 0;  // +0 / -0 are "drop", like != 0
    default: return ((const uint8_t*)mask)[at] != 0;
  }
}

__global__ __launch_bounds__(kRsThreads) void expand_count_kernel(const void* __restrict__ mask, int mask_dtype, int64_t P,
                                                                  int n_per, int32_t* __restrict__ cnt,
                                                                  int32_t* __restrict__ tile) {
  const int64_t p = (int64_t)blockIdx.x * kRsThreads + threadIdx.x;
  int c = 0;
  if (p < P) {
    for (int s = 0; s < n_per; ++s) c += mask_keeps(mask, mask_dtype, p * n_per + s) ? 1 : 0;
    cnt[p] = c;
  }
  __shared__ int s_w[kRsThreads / 64];
  int total;
  block_excl_scan<kRsThreads>(c, s_w, &total);
  if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

// one workgroup: tile counts -> exclusive prefix in place (tile[T] = total); out_offsets[b] = children of the parents whose
// batch index is < b (parents are batch-sorted: the boundary row by bisection, then the counts of its tile in front of it)
__global__ __launch_bounds__(kRsThreads) void expand_scan_kernel(int32_t* __restrict__ tile, int64_t T,
                                                                 const int32_t* __restrict__ cnt, int64_t P,
                                                                 const int4* __restrict__ parents, int num_batches,
                                                                 int32_t* __restrict__ out_offsets) {
  __shared__ int s_w[kRsThreads / 64];
  int carry = 0;
  for (int64_t base = 0; base < T; base += kRsThreads) {
    const int64_t e = base + threadIdx.x;
    const int v = e < T ? tile[e] : 0;
    int total;
    const int excl = block_excl_scan<kRsThreads>(v, s_w, &total);
    if (e < T) tile[e] = carry + excl;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) tile[T] = carry;
  __syncthreads();
  for (int b = threadIdx.x; b <= num_batches; b += kRsThreads) {
    const int64_t lo = first_row_of_batch(parents, P, b);
    const int64_t r = b >= num_batches ? P : lo;
    int v = carry;
    if (r < P) {
      const int64_t t = r / kRsThreads;
      v = tile[t];
      for (int64_t i = t * kRsThreads; i < r; ++i) v += cnt[i];
    }
    out_offsets[b] = v;
  }
}

__global__ __launch_bounds__(kRsThreads) void expand_emit_kernel(const int4* __restrict__ parents, const void* __restrict__ mask,
                                                                 int mask_dtype, int64_t P, int n_per, int factor, int z_fastest,
                                                                 const int32_t* __restrict__ cnt, const int32_t* __restrict__ tile,
                                                                 int64_t capacity, int4* __restrict__ child_coords,
                                                                 int32_t* __restrict__ tbl, int pitch) {
  const int64_t p = (int64_t)blockIdx.x * kRsThreads + threadIdx.x;
  const int c = p < P ? cnt[p] : 0;
  __shared__ int s_w[kRsThreads / 64];
  int total;
  int64_t pos = (int64_t)tile[blockIdx.x] + block_excl_scan<kRsThreads>(c, s_w, &total);
  if (p >= P) return;
  const int4 pc = parents[p];
  const int f2 = factor * factor;
  for (int s = 0; s < n_per; ++s) {
    int32_t row = -1;
    if (mask_keeps(mask, mask_dtype, p * n_per + s) && pos < capacity) {
      const int a = s % factor, b = (s / factor) % factor, d = s / f2;  // column s -> offset inside the parent cell
      const int ox = z_fastest ? d : a, oz = z_fastest ? a : d;
      if (child_coords) child_coords[pos] = make_int4(pc.x, pc.y * factor + ox, pc.z * factor + b, pc.w * factor + oz);
      row = (int32_t)pos;
      ++pos;
    }
    if (tbl) tbl[p * pitch + s] = row;
  }
  if (tbl)
    for (int s = n_per; s < pitch; ++s) tbl[p * pitch + s] = -1;
}

}  // namespace wcn

using namespace wcn;

extern "C" {

int wcn_resample_pack(const void* src, const int32_t* tbl, int64_t n_src, int64_t n_parent, int32_t channels, int32_t n_per,
                      int32_t factor, int32_t pitch, int32_t slot_order, int32_t dtype, void* dst, wcn_stream_t stream) {
  if (n_src < 0 || n_parent < 0 || channels < 1 || n_per < 1 || pitch < n_per) return WCN_ERROR_INVALID_PARAMETERS;
  const int eb = dtype_ok(dtype) ? dtype_bytes(dtype) : 0;
  SlotCols sc;
  if (!eb || n_per > kRsMaxPer || !slot_cols(n_per, factor, slot_order, &sc)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if ((int64_t)channels * n_per * eb > (1ll << 24)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (n_parent == 0) return WCN_SUCCESS;
  if (!tbl || !dst || (n_src > 0 && !src)) return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  const int row_bytes = channels * eb;
  if (row_bytes % 16 == 0 && aligned_to(src, 16) && aligned_to(dst, 16))
    return pack_u<uint4>(src, tbl, n_src, n_parent, n_per, pitch, sc, row_bytes / 16, dst, s);
  if (eb == 4) return pack_u<uint32_t>(src, tbl, n_src, n_parent, n_per, pitch, sc, channels, dst, s);
  return pack_u<uint16_t>(src, tbl, n_src, n_parent, n_per, pitch, sc, channels, dst, s);
}

int wcn_resample_unpack(const void* src, const int32_t* tbl, int64_t n_parent, int64_t n_dst, int32_t channels, int32_t n_per,
                        int32_t factor, int32_t pitch, int32_t slot_order, int32_t broadcast, int32_t dtype, void* dst,
                        wcn_stream_t stream) {
  if (n_dst < 0 || n_parent < 0 || channels < 1 || n_per < 1 || (tbl && pitch < n_per)) return WCN_ERROR_INVALID_PARAMETERS;
  const int eb = dtype_ok(dtype) ? dtype_bytes(dtype) : 0;
  SlotCols sc;
  if (!eb || n_per > kRsMaxPer || !slot_cols(n_per, factor, slot_order, &sc)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if ((int64_t)channels * n_per * eb > (1ll << 24)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (n_parent == 0 || n_dst == 0) return WCN_SUCCESS;
  if (!src || !dst) return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  const int row_bytes = channels * eb;
  const int bc = broadcast ? 1 : 0;
  if (row_bytes % 16 == 0 && aligned_to(src, 16) && aligned_to(dst, 16))
    return unpack_u<uint4>(src, tbl, n_parent, n_dst, n_per, pitch, sc, row_bytes / 16, bc, dst, s);
  if (eb == 4) return unpack_u<uint32_t>(src, tbl, n_parent, n_dst, n_per, pitch, sc, channels, bc, dst, s);
  return unpack_u<uint16_t>(src, tbl, n_parent, n_dst, n_per, pitch, sc, channels, bc, dst, s);
}

size_t wcn_resample_expand_workspace(int64_t n_parent) {
  const int64_t P = n_parent > 0 ? n_parent : 0;
  return (size_t)(((P + 3) & ~(int64_t)3) + expand_tiles(P) + 4) * sizeof(int32_t);
}

int wcn_resample_expand(const int32_t* parents, const void* mask, int32_t mask_dtype, int64_t n_parent, int32_t n_per,
                        int32_t factor, int32_t slot_order, int32_t num_batches, void* workspace, size_t workspace_bytes,
                        int32_t* out_offsets, int64_t capacity, int32_t* child_coords, int32_t* tbl, int32_t pitch,
                        wcn_stream_t stream) {
  if (n_parent < 0 || num_batches < 0 || capacity < 0 || n_parent >= (1ll << 31) / kRsMaxPer)
    return WCN_ERROR_INVALID_PARAMETERS;
  if (mask_dtype < 0 || mask_dtype > kRsMaskU8) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (slot_order != WCN_SLOT_X_FASTEST && slot_order != WCN_SLOT_Z_FASTEST) return WCN_ERROR_INVALID_PARAMETERS;
  if (factor < 1 || factor > 4 || !(n_per == factor * factor * factor || (n_per == 1 && factor == 1)))
    return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (!workspace || workspace_bytes < wcn_resample_expand_workspace(n_parent)) return WCN_ERROR_INVALID_PARAMETERS;
  if (n_parent > 0 && !parents) return WCN_ERROR_INVALID_PARAMETERS;
  if (tbl && pitch < n_per) return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  const ExpandWs w = carve_expand(workspace, n_parent);
  const int64_t T = expand_tiles(n_parent);
  if (out_offsets) {  // phase 1: count + scan
    if (T > 0)
      hipLaunchKernelGGL(expand_count_kernel, dim3((unsigned)T), dim3(kRsThreads), 0, s, mask, (int)mask_dtype, n_parent,
                         (int)n_per, w.cnt, w.tile);
    hipLaunchKernelGGL(expand_scan_kernel, dim3(1), dim3(kRsThreads), 0, s, w.tile, T, w.cnt, n_parent, (const int4*)parents,
                       (int)num_batches, out_offsets);
  }
  if ((child_coords || tbl) && T > 0)  // phase 2: emit, from the workspace phase 1 left
    hipLaunchKernelGGL(expand_emit_kernel, dim3((unsigned)T), dim3(kRsThreads), 0, s, (const int4*)parents, mask, (int)mask_dtype,
                       n_parent, (int)n_per, (int)factor, slot_order == WCN_SLOT_Z_FASTEST ? 1 : 0, w.cnt, w.tile, capacity,
                       (int4*)child_coords, tbl, (int)pitch);
  return launch_status();
}

}  // extern "C"
