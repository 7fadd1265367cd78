// voxelize.hip - points <-> voxels: the map of a point cloud onto its voxels and the two feature kernels that run over it
// (reference: nn/functional/point_pool.py, point_unpool.py and utils/unique.py, where the same steps are torch.unique over
// rows, an argsort, a materialised features[perm] and torch_scatter.segment_csr).
//
//   a. wcn_voxel_keys         one packed int64 key per point: batch << 54 | (x + 2^17) << 36 | (y + 2^17) << 18 | (z + 2^17),
//                             the biased 18-bit fields of wcn_common.h, so that int64 order = lexicographic order of the
//                             signed (b, x, y, z) rows.  The stable sort of the keys is the caller's (framework radix sort).
//   b. wcn_voxel_map          sorted keys + permutation -> unique keys / coordinates, CSR offsets, voxel of every point,
//                             first point of every voxel, voxel offsets per batch element, (M, longest segment): the
//                             runs -> map kernels of row_lists.h on int64 keys.
//   c. wcn_csr_gather_reduce  out[m] = op over j in [offsets[m], offsets[m + 1]) of in[indices[j]]: pool forward, unpool
//                             backward.  Lanes run along channels (16-B / 8-B / element pieces), a group of lanes owns one
//                             segment and adds its rows in ascending j; narrow rows put 64 / group segments in one wave.
//                             Segments longer than kRowChunk rows go by the chunk rule of row_lists.h: the bits of a row
//                             depend on the segment alone, never on the launch shape or the path taken.
//   d. wcn_row_spread         out[i, :c] = scale(i) * src[to_orig[i]], out[i, c:c + cs] = skip[i]: unpool forward (with the
//                             concatenation in the same pass), pool backward (1 / count, or the arg-match of max / min).
// No float atomics anywhere; the integer atomics (status word, longest segment, the list of long segments) give the same
// result in any order.  Every grid is capped at kRowMaxGrid workgroups and strides.

#include <cfloat>

#include "row_lists.h"

namespace wcn {

constexpr int64_t kCoordBias = -(int64_t)kCoordMin;

enum { kVxFlagRange = 1, kVxFlagOffsets = 2 };
enum { kOpSum = 0, kOpMean = 1, kOpMax = 2, kOpMin = 3 };
enum { kSpreadPlain = 0, kSpreadInvCount = 1, kSpreadArgMatch = 2 };

// ---- a. keys ----------------------------------------------------------------------------------------------------------------
// cell = floor(p * inv_voxel_size), the reciprocal formed by the CALLER: the framework evaluates `points / voxel_size` for a
// host scalar on the device as a product with fp32(1.0 / voxel_size), the quotient taken in double (measured, DESIGN.md
// "Quantisation finding"), and a point on a cell face lands in another cell under a true division or a reciprocal rounded
// differently.  A cell outside the 18-bit range (NaN included) or a row that belongs to no batch element raises the status.
__global__ __launch_bounds__(kRowThreads) void vx_keys_kernel(const float* __restrict__ points, int64_t n,
                                                             const int32_t* __restrict__ batch_offsets, int num_batches,
                                                             float inv, int64_t* __restrict__ keys,
                                                             int32_t* __restrict__ status) {
  for (int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRowThreads) {
    int b = 0, hi = num_batches;
    while (b < hi) {
      const int mid = (b + hi) >> 1;
      if (i < batch_offsets[mid + 1]) hi = mid; else b = mid + 1;
    }
    if (b >= num_batches || i < batch_offsets[0]) {
      keys[i] = -1;
      atomicOr(status, kVxFlagOffsets);
      continue;
    }
    const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
    const float fx = floorf(px * inv), fy = floorf(py * inv), fz = floorf(pz * inv);
    const float lo = (float)kCoordMin, up = (float)kCoordMax;
    if (!(fx >= lo && fx <= up && fy >= lo && fy <= up && fz >= lo && fz <= up)) {
      keys[i] = -1;
      atomicOr(status, kVxFlagRange);
      continue;
    }
    keys[i] = ((int64_t)b << 54) | (((int64_t)fx + kCoordBias) << 36) | (((int64_t)fy + kCoordBias) << 18) |
              ((int64_t)fz + kCoordBias);
  }
}

// ---- b. runs -> map ---------------------------------------------------------------------------------------------------------
struct VxKeys {  // key policy of row_lists.h: one int64 per position
  using Key = int64_t;
  const int64_t* keys;
  __device__ __forceinline__ void load(int64_t n, int64_t i0, Key (&k)[kRunPer]) const {
    if (i0 + kRunPer <= n) {
      const longlong2* p = reinterpret_cast<const longlong2*>(keys + i0);  // i0 is a multiple of 8, keys 16-B aligned
#pragma unroll
      for (int j = 0; j < kRunPer; j += 2) {
        const longlong2 q = p[j >> 1];
        k[j] = q.x;
        k[j + 1] = q.y;
      }
    } else {
#pragma unroll
      for (int j = 0; j < kRunPer; ++j) k[j] = i0 + j < n ? keys[i0 + j] : 0;
    }
  }
  __device__ __forceinline__ Key at(int64_t i) const { return keys[i]; }
  static __device__ __forceinline__ bool differ(Key a, Key b) { return a != b; }
};

struct VxWriter {  // what a voxel and a point get
  int64_t* unique_keys;
  int32_t* unique_coords;  // optional
  int64_t* to_orig;
  int64_t* to_unique;
  __device__ __forceinline__ void head(int64_t vid, int64_t row, int64_t key) const {
    unique_keys[vid] = key;
    to_unique[vid] = row;  // stable sort: the first position of a run holds the run's smallest row
    if (unique_coords) {
      unique_coords[3 * vid] = (int32_t)(((key >> 36) & kCoordMask) - kCoordBias);
      unique_coords[3 * vid + 1] = (int32_t)(((key >> 18) & kCoordMask) - kCoordBias);
      unique_coords[3 * vid + 2] = (int32_t)((key & kCoordMask) - kCoordBias);
    }
  }
  __device__ __forceinline__ void each(int64_t row, int64_t vid) const { to_orig[row] = vid; }
};

// per voxel: the longest segment (integer atomic max) and, where the batch field of the key steps, the voxel offsets of the
// batch elements in between (every word written once: voxels are key-sorted, so the batch field ascends)
__global__ __launch_bounds__(kRowThreads) void vx_finish_kernel(const int64_t* __restrict__ unique_keys,
                                                               const int64_t* __restrict__ csr_offsets, int64_t n,
                                                               int32_t* __restrict__ summary,
                                                               int32_t* __restrict__ batch_voxel_offsets, int num_batches) {
  int64_t M = summary[0];
  if (M > n) M = n;
  int longest = 0;
  for (int64_t v = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; v < M; v += (int64_t)gridDim.x * kRowThreads) {
    longest = max(longest, row_length(csr_offsets, v));
    if (batch_voxel_offsets) {
      int b = (int)(unique_keys[v] >> 54);
      b = b < 0 ? 0 : (b > num_batches - 1 ? num_batches - 1 : b);
      const int before = v > 0 ? (int)(unique_keys[v - 1] >> 54) : -1;
      for (int q = max(before, -1) + 1; q <= b; ++q) batch_voxel_offsets[q] = (int32_t)v;
      if (v == M - 1)
        for (int q = b + 1; q <= num_batches; ++q) batch_voxel_offsets[q] = (int32_t)M;
    }
  }
  longest_row_max(longest, summary + 1);
}

// ---- c. CSR gather-reduce ---------------------------------------------------------------------------------------------------
struct CgLong : RowList {  // the long segments and their chunks, listed per call, and the chunks' partials
  float* part;        // [item_cap][c]
  int64_t* part_arg;  // [item_cap][c] (max / min)
  size_t bytes;
};

// the list and the partials in the byte workspace, every array 256-B aligned
static CgLong cg_carve(void* base, int64_t nnz, int64_t c, bool with_arg) {
  CgLong w;
  row_list_caps(nnz, w);
  char* p = (char*)base;
  size_t at = 0;
  w.counters = (int32_t*)(p + at);
  at = align256(at + kRowListCounterInts * 4);
  w.item_row = (int32_t*)(p + at);
  at = align256(at + (size_t)w.item_cap * 4);
  w.item_k = (int32_t*)(p + at);
  at = align256(at + (size_t)w.item_cap * 4);
  w.long_row = (int32_t*)(p + at);
  at = align256(at + (size_t)w.long_cap * 4);
  w.long_base = (int32_t*)(p + at);
  at = align256(at + (size_t)w.long_cap * 4);
  w.part = (float*)(p + at);
  at = align256(at + (size_t)w.item_cap * c * 4);
  w.part_arg = (int64_t*)(p + at);
  if (with_arg) at = align256(at + (size_t)w.item_cap * c * 8);
  w.bytes = at;
  return w;
}

// rows [j0, j1) of one list, ascending, into acc (and the first extremum's row into best); `col` .. col + V - 1 of every row
template <typename T, int V>
__device__ __forceinline__ void cg_rows(const T* __restrict__ in, int64_t ld_in, int64_t n_in,
                                        const int64_t* __restrict__ indices, int64_t j0, int64_t j1, int col, int op,
                                        float (&acc)[V], int64_t (&best)[V]) {
  auto take = [&](int64_t row, const float (&f)[V]) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (op == kOpMax) {
        if (best[e] < 0 || f[e] > acc[e]) { acc[e] = f[e]; best[e] = row; }
      } else if (op == kOpMin) {
        if (best[e] < 0 || f[e] < acc[e]) { acc[e] = f[e]; best[e] = row; }
      } else {
        acc[e] += f[e];
      }
    }
  };
  int64_t j = j0;
  for (; j + 4 <= j1; j += 4) {  // four rows in flight, added in order
    int64_t r[4];
    float f[4][V];
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = indices ? indices[j + u] : j + u;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (r[u] >= 0 && r[u] < n_in) {
        ld_vec<T, V>(in + r[u] * ld_in + col, f[u]);
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) f[u][e] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) take(r[u], f[u]);
  }
  for (; j < j1; ++j) {
    const int64_t r = indices ? indices[j] : j;
    float f[V];
    if (r >= 0 && r < n_in) {
      ld_vec<T, V>(in + r * ld_in + col, f);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) f[e] = 0.f;
    }
    take(r, f);
  }
}

// L lanes (a power of two <= 64) own one list: ITEMS = false, a whole segment (longer ones are skipped when `split`);
// ITEMS = true, one chunk of a long segment into the fp32 partials.  Rows wider than L * V channels take several trips.
template <typename T, int V, bool ITEMS>
__global__ __launch_bounds__(kRowThreads) void cg_reduce_kernel(const T* __restrict__ in, int64_t ld_in,
                                                               int64_t n_in, const int64_t* __restrict__ indices,
                                                               const int64_t* __restrict__ offsets, int64_t m, int64_t nnz,
                                                               int c, int L, int op, int split,
                                                               T* __restrict__ out, int64_t* __restrict__ arg,
                                                               CgLong w) {
  const int groups = kRowThreads / L;
  const int g = threadIdx.x / L, sub = threadIdx.x % L;
  const int64_t total = ITEMS ? row_list_items(w) : m;
  for (int64_t t = (int64_t)blockIdx.x * groups + g; t < total; t += (int64_t)gridDim.x * groups) {
    int64_t seg = t, j0, j1;
    if (!(ITEMS ? row_list_item(w, t, offsets, m, nnz, seg, j0, j1) : row_span(offsets, m, nnz, seg, j0, j1))) continue;
    const int64_t len = j1 - j0;  // of the whole segment where it is used
    if (!ITEMS && split && len > kRowChunk) continue;
    for (int col = sub * V; col < c; col += L * V) {
      float acc[V];
      int64_t best[V];
#pragma unroll
      for (int e = 0; e < V; ++e) { acc[e] = 0.f; best[e] = -1; }
      cg_rows<T, V>(in, ld_in, n_in, indices, j0, j1, col, op, acc, best);
      if (ITEMS) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          w.part[t * c + col + e] = acc[e];
          if (op >= kOpMax) w.part_arg[t * c + col + e] = best[e];
        }
      } else {
        if (op == kOpMean && len > 0) {
#pragma unroll
          for (int e = 0; e < V; ++e) acc[e] /= (float)len;
        }
        st_vec<T, V>(out + seg * c + col, acc);
        if (arg) {
#pragma unroll
          for (int e = 0; e < V; ++e) arg[seg * c + col + e] = best[e];
        }
      }
    }
  }
}

// L lanes per long segment: its partials in chunk order
template <typename T>
__global__ __launch_bounds__(kRowThreads) void cg_combine_kernel(const int64_t* __restrict__ offsets, int64_t m, int c, int L,
                                                                int op, T* __restrict__ out,
                                                                int64_t* __restrict__ arg, CgLong w) {
  const int groups = kRowThreads / L;
  const int g = threadIdx.x / L, sub = threadIdx.x % L;
  const int64_t total = row_list_long_rows(w);
  for (int64_t t = (int64_t)blockIdx.x * groups + g; t < total; t += (int64_t)gridDim.x * groups) {
    int64_t seg, len, first, nch;
    if (!row_list_long_row(w, t, offsets, m, seg, len, first, nch)) continue;
    for (int col = sub; col < c; col += L) {
      float acc = w.part[first * c + col];
      int64_t best = op >= kOpMax ? w.part_arg[first * c + col] : -1;
      for (int64_t k = 1; k < nch; ++k) {
        const float f = w.part[(first + k) * c + col];
        if (op == kOpMax) {
          if (f > acc) { acc = f; best = w.part_arg[(first + k) * c + col]; }
        } else if (op == kOpMin) {
          if (f < acc) { acc = f; best = w.part_arg[(first + k) * c + col]; }
        } else {
          acc += f;
        }
      }
      if (op == kOpMean) acc /= (float)len;
      out[seg * c + col] = (T)acc;
      if (arg) arg[seg * c + col] = best;
    }
  }
}

template <typename T, int V>
static void cg_launch(const void* in, int64_t ld_in, int64_t n_in, const int64_t* indices, const int64_t* offsets, int64_t m,
                      int64_t nnz, int c, int op, bool split, void* out, int64_t* arg, const CgLong& w, hipStream_t s) {
  const int L = row_lanes(ceil_div(c, V)), groups = kRowThreads / L;
  hipLaunchKernelGGL((cg_reduce_kernel<T, V, false>), dim3(capped_grid(ceil_div(m, groups))), dim3(kRowThreads), 0, s,
                     (const T*)in, ld_in, n_in, indices, offsets, m, nnz, c, L, op, split ? 1 : 0, (T*)out, arg, w);
  if (!split) return;
  hipLaunchKernelGGL(row_list_collect_kernel<>, dim3(capped_grid(ceil_div(m, kRowThreads))), dim3(kRowThreads), 0, s, offsets, m,
                     nnz, (const RowList&)w);
  hipLaunchKernelGGL((cg_reduce_kernel<T, V, true>), dim3(capped_grid(ceil_div(w.item_cap, groups))), dim3(kRowThreads), 0, s,
                     (const T*)in, ld_in, n_in, indices, offsets, m, nnz, c, L, op, 1, (T*)out, arg, w);
  const int Lc = row_lanes(c);
  hipLaunchKernelGGL(cg_combine_kernel<T>, dim3(capped_grid(ceil_div(w.long_cap, kRowThreads / Lc))), dim3(kRowThreads), 0, s,
                     offsets, m, c, Lc, op, (T*)out, arg, w);
}

// widest piece (elements per lane) that the channel count, the row strides and the pointers allow: 16 B, 8 B or one element
static int piece_elems(int dtype, int64_t c, int64_t c2, int64_t ld_a, int64_t ld_b, const void* p0, const void* p1,
                       const void* p2) {
  const int es = dtype_bytes(dtype);
  for (int bytes = 16; bytes >= 8; bytes >>= 1) {
    const int v = bytes / es;
    if (c % v == 0 && c2 % v == 0 && ld_a % v == 0 && ld_b % v == 0 && aligned_to(p0, bytes) && aligned_to(p1, bytes) &&
        aligned_to(p2, bytes))
      return v;
  }
  return 1;
}

// ---- d. indexed row spread --------------------------------------------------------------------------------------------------
// one thread per V-element piece of an output row: the first c / V pieces come from src[to_orig[i]], the next cs / V from skip[i]
template <typename T, int V>
__global__ __launch_bounds__(kRowThreads) void row_spread_kernel(const T* __restrict__ src,
                                                                const int64_t* __restrict__ to_orig, int64_t n, int64_t m,
                                                                int c, const T* __restrict__ skip, int cs,
                                                                int64_t ld_out, int mode, const int64_t* __restrict__ offsets,
                                                                const int64_t* __restrict__ arg,
                                                                T* __restrict__ out) {
  const int pc = c / V, pw = pc + cs / V;
  const int64_t total = n * pw;
  for (int64_t e = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kRowThreads) {
    const int64_t i = e / pw;
    const int p = (int)(e - i * pw);
    float f[V];
    if (p >= pc) {
      const int col = (p - pc) * V;
      // the piece as it is: through floats the compiler merges this store with the one below and splits both
      *reinterpret_cast<Vec<T, V>*>(out + i * ld_out + c + col) = *reinterpret_cast<const Vec<T, V>*>(skip + i * cs + col);
      continue;
    }
    const int col = p * V;
    const int64_t v = to_orig[i];
    if (v < 0 || v >= m) {
#pragma unroll
      for (int q = 0; q < V; ++q) f[q] = 0.f;
    } else {
      ld_vec<T, V>(src + v * c + col, f);
      if (mode == kSpreadInvCount) {
        const int64_t len = offsets[v + 1] - offsets[v];
        const float cnt = (float)(len > 0 ? len : 1);
#pragma unroll
        for (int q = 0; q < V; ++q) f[q] /= cnt;
      } else if (mode == kSpreadArgMatch) {
#pragma unroll
        for (int q = 0; q < V; ++q) f[q] = arg[v * c + col + q] == i ? f[q] : 0.f;
      }
    }
    st_vec<T, V>(out + i * ld_out + col, f);
  }
}

template <typename T, int V>
static void spread_launch(const void* src, const int64_t* to_orig, int64_t n, int64_t m, int c, const void* skip, int cs,
                          int64_t ld_out, int mode, const int64_t* offsets, const int64_t* arg, void* out, hipStream_t s) {
  const int64_t pieces = n * (int64_t)((c + cs) / V);
  hipLaunchKernelGGL((row_spread_kernel<T, V>), dim3(capped_grid(ceil_div(pieces, kRowThreads))), dim3(kRowThreads), 0, s,
                     (const T*)src, to_orig, n, m, c, (const T*)skip, cs, ld_out, mode, offsets, arg, (T*)out);
}

}  // namespace wcn

using namespace wcn;

extern "C" {

int32_t wcn_csr_chunk_rows(void) { return kRowChunk; }

int wcn_voxel_keys(const float* points, int64_t n, const int32_t* batch_offsets, int32_t num_batches, float inv_voxel_size,
                   int64_t* keys, int32_t* status, wcn_stream_t stream) {
  if (n < 0 || n > INT32_MAX || !status) return WCN_ERROR_INVALID_PARAMETERS;
  if (points && (num_batches < 1 || num_batches > kBatchMax + 1 || !(inv_voxel_size > 0.f) || !(inv_voxel_size < FLT_MAX)))
    return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, 4, s) != hipSuccess) return WCN_ERROR_KERNEL_EXECUTION;
  if (n == 0 || !points) return WCN_SUCCESS;  // null points: the keys are the caller's own codes
  if (!batch_offsets || !keys) return WCN_ERROR_INVALID_PARAMETERS;
  hipLaunchKernelGGL(vx_keys_kernel, dim3(capped_grid(ceil_div(n, kRowThreads))), dim3(kRowThreads), 0, s, points, n, batch_offsets,
                     (int)num_batches, inv_voxel_size, keys, status);
  return launch_status();
}

size_t wcn_voxel_map_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return align256((size_t)ceil_div(n > 0 ? n : 1, kRunTile) * 4);
}

int wcn_voxel_map(const int64_t* sorted_keys, const int64_t* perm, int64_t n, int32_t num_batches, int64_t* unique_keys,
                  int32_t* unique_coords, int64_t* csr_offsets, int64_t* to_orig, int64_t* to_unique,
                  int32_t* batch_voxel_offsets, int32_t* summary, void* workspace, size_t workspace_bytes,
                  wcn_stream_t stream) {
  if (n < 0 || n > INT32_MAX || !summary || !csr_offsets || num_batches < 0 || num_batches > kBatchMax + 1 ||
      (batch_voxel_offsets && num_batches < 1))
    return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  if (n > 0 && (!sorted_keys || !perm || !unique_keys || !to_orig || !to_unique || !workspace ||
                !aligned_to(sorted_keys, 16) || !aligned_to(workspace, 16) ||
                workspace_bytes < wcn_voxel_map_workspace_bytes(n)))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (hipMemsetAsync(summary, 0, 8, s) != hipSuccess || hipMemsetAsync(csr_offsets, 0, 8, s) != hipSuccess)
    return WCN_ERROR_KERNEL_EXECUTION;
  if (batch_voxel_offsets && hipMemsetAsync(batch_voxel_offsets, 0, ((size_t)num_batches + 1) * 4, s) != hipSuccess)
    return WCN_ERROR_KERNEL_EXECUTION;
  if (n == 0) return WCN_SUCCESS;
  const int64_t ntiles = ceil_div(n, kRunTile);
  int32_t* tile_sum = (int32_t*)workspace;
  const dim3 block(kRowThreads), tiles(capped_grid(ntiles));
  const VxKeys keys{sorted_keys};
  hipLaunchKernelGGL(run_count_kernel<VxKeys>, tiles, block, 0, s, keys, n, ntiles, tile_sum);
  hipLaunchKernelGGL(run_scan_kernel<>, dim3(1), block, 0, s, tile_sum, ntiles, n, summary, csr_offsets);
  hipLaunchKernelGGL((run_apply_kernel<VxKeys, VxWriter>), tiles, block, 0, s, keys, perm, n, ntiles, (const int32_t*)tile_sum,
                     csr_offsets, VxWriter{unique_keys, unique_coords, to_orig, to_unique});
  hipLaunchKernelGGL(vx_finish_kernel, dim3(capped_grid(ceil_div(n, kRowThreads))), block, 0, s, unique_keys, csr_offsets, n,
                     summary, batch_voxel_offsets, (int)num_batches);
  return launch_status();
}

static int cg_args_ok(int64_t m, int64_t nnz, int64_t n_in, int32_t c, int64_t ld, int32_t dtype, int32_t op) {
  if (m < 0 || m > INT32_MAX || nnz < 0 || nnz > INT32_MAX || n_in < 0 || c < 0 || ld < c || op < kOpSum || op > kOpMin)
    return WCN_ERROR_INVALID_PARAMETERS;
  if (!dtype_ok(dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  return WCN_SUCCESS;
}

size_t wcn_csr_gather_reduce_workspace_bytes(int64_t nnz, int32_t c, int32_t op) {
  if (nnz < 0 || c < 0) return 0;
  return cg_carve(nullptr, nnz, c, op >= kOpMax).bytes;
}

int wcn_csr_gather_reduce(const void* in, int64_t ld_in, int64_t n_in, const int64_t* indices, const int64_t* offsets,
                          int64_t m, int64_t nnz, int32_t c, int32_t dtype, int32_t op, int64_t max_segment, void* out,
                          int64_t* arg, void* workspace, size_t workspace_bytes, wcn_stream_t stream) {
  const int st = cg_args_ok(m, nnz, n_in, c, ld_in, dtype, op);
  if (st != WCN_SUCCESS) return st;
  if (m == 0 || c == 0) return WCN_SUCCESS;
  if (!offsets || !out || (!in && nnz > 0) || (arg && op < kOpMax)) return WCN_ERROR_INVALID_PARAMETERS;
  const bool split = max_segment < 0 || max_segment > kRowChunk;  // < 0: the caller does not know the longest segment
  CgLong w{};
  hipStream_t s = (hipStream_t)stream;
  if (split) {
    if (!workspace || !aligned_to(workspace, 16)) return WCN_ERROR_INVALID_PARAMETERS;
    w = cg_carve(workspace, nnz, c, op >= kOpMax);
    if (workspace_bytes < w.bytes) return WCN_ERROR_INVALID_PARAMETERS;
    if (hipMemsetAsync(w.counters, 0, kRowListCounterInts * 4, s) != hipSuccess) return WCN_ERROR_KERNEL_EXECUTION;
  }
  const int v = piece_elems(dtype, c, 0, ld_in, 0, in, out, nullptr);
  with_dtype_vec<true>(dtype, v, [&](auto t, auto vc) {
    cg_launch<decltype(t), vc()>(in, ld_in, n_in, indices, offsets, m, nnz, (int)c, (int)op, split, out, arg, w, s);
    return 0;
  });
  return launch_status();
}

int wcn_row_spread(const void* src, const int64_t* to_orig, int64_t n, int64_t m, int32_t c, const void* skip, int32_t cs,
                   int64_t ld_out, int32_t mode, const int64_t* offsets, const int64_t* arg, int32_t dtype, void* out,
                   wcn_stream_t stream) {
  if (n < 0 || n > INT32_MAX || m < 0 || m > INT32_MAX || c < 0 || cs < 0 || ld_out < (int64_t)c + cs ||
      mode < kSpreadPlain || mode > kSpreadArgMatch)
    return WCN_ERROR_INVALID_PARAMETERS;
  if (!dtype_ok(dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (n == 0 || c + cs == 0) return WCN_SUCCESS;
  if (!out || (c > 0 && (!to_orig || (!src && m > 0))) || (cs > 0 && !skip) || (mode == kSpreadInvCount && !offsets) ||
      (mode == kSpreadArgMatch && !arg))
    return WCN_ERROR_INVALID_PARAMETERS;
  const int v = piece_elems(dtype, c, cs, ld_out, 0, src, skip, out);
  with_dtype_vec<true>(dtype, v, [&](auto t, auto vc) {
    spread_launch<decltype(t), vc()>(src, to_orig, n, m, (int)c, skip, (int)cs, ld_out, (int)mode, offsets, arg, out,
                                     (hipStream_t)stream);
    return 0;
  });
  return launch_status();
}

}  // extern "C"
