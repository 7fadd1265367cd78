// voxelize.hip - points <-> voxels: the map of a point cloud onto its voxels and the two feature kernels that run over it
// (reference: nn/functional/point_pool.py, point_unpool.py and utils/unique.py, where the same steps are torch.unique over
// rows, an argsort, a materialised features[perm] and torch_scatter.segment_csr).
//
//   a. wcn_voxel_keys         one packed int64 key per point: batch << 54 | (x + 2^17) << 36 | (y + 2^17) << 18 | (z + 2^17),
//                             the biased 18-bit fields of wcn_common.h, so that int64 order = lexicographic order of the
//                             signed (b, x, y, z) rows.  The stable sort of the keys is the caller's (framework radix sort).
//   b. wcn_voxel_map          sorted keys + permutation -> unique keys / coordinates, CSR offsets, voxel of every point,
//                             first point of every voxel, voxel offsets per batch element, (M, longest segment).  Run heads
//                             are counted per 2048-key tile, ONE workgroup scans the tile sums, the tiles are applied:
//                             no kernel waits on another workgroup.
//   c. wcn_csr_gather_reduce  out[m] = op over j in [offsets[m], offsets[m + 1]) of in[indices[j]]: pool forward, unpool
//                             backward.  Lanes run along channels (16-B / 8-B / element pieces), a group of lanes owns one
//                             segment and adds its rows in ascending j; narrow rows put 64 / group segments in one wave.
//                             Segments longer than kCgChunk rows are cut into chunks of kCgChunk rows, each summed the same
//                             way by its own group into an fp32 partial, and the partials are added in chunk order: the
//                             bits of a row depend on the segment alone, never on the launch shape or the path taken.
//   d. wcn_row_spread         out[i, :c] = scale(i) * src[to_orig[i]], out[i, c:c + cs] = skip[i]: unpool forward (with the
//                             concatenation in the same pass), pool backward (1 / count, or the arg-match of max / min).
// No float atomics anywhere; the integer atomics (status word, longest segment, the list of long segments) give the same
// result in any order.  Every grid is capped at kVxMaxGrid workgroups and strides.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cfloat>
#include <limits.h>

#include "wcn_common.h"

namespace wcn {

constexpr int kVxThreads = 256;
constexpr int kVxPer = 8;
constexpr int kVxTile = kVxThreads * kVxPer;  // sorted keys of one scan tile
constexpr int kVxMaxGrid = 4096;
constexpr int kCgChunk = 256;                 // rows of one chunk of a long segment (the chunk rule)
constexpr int kCgCounterInts = 64;            // [0] chunk items, [1] long segments; padded to 256 B
constexpr int64_t kCoordBias = -(int64_t)kCoordMin;

enum { kVxFlagRange = 1, kVxFlagOffsets = 2 };
enum { kOpSum = 0, kOpMean = 1, kOpMax = 2, kOpMin = 3 };
enum { kSpreadPlain = 0, kSpreadInvCount = 1, kSpreadArgMatch = 2 };

static unsigned vx_grid(int64_t items) {
  const int64_t g = items < 1 ? 1 : items;
  return (unsigned)(g < kVxMaxGrid ? g : kVxMaxGrid);
}

// ---- a. keys ----------------------------------------------------------------------------------------------------------------
// cell = floor(p * inv_voxel_size), the reciprocal formed by the CALLER: the framework evaluates `points / voxel_size` for a
// host scalar on the device as a product with fp32(1.0 / voxel_size), the quotient taken in double (measured, DESIGN.md
// "Quantisation finding"), and a point on a cell face lands in another cell under a true division or a reciprocal rounded
// differently.  A cell outside the 18-bit range (NaN included) or a row that belongs to no batch element raises the status.
__global__ __launch_bounds__(kVxThreads) void vx_keys_kernel(const float* __restrict__ points, int64_t n,
                                                             const int32_t* __restrict__ batch_offsets, int num_batches,
                                                             float inv, int64_t* __restrict__ keys,
                                                             int32_t* __restrict__ status) {
  for (int64_t i = (int64_t)blockIdx.x * kVxThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kVxThreads) {
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
// thread t of a tile owns the sorted positions tile * kVxTile + t * kVxPer .. + kVxPer - 1; head = first position of a run
__device__ __forceinline__ int vx_load_heads(const int64_t* __restrict__ keys, int64_t n, int64_t i0, int64_t (&k)[kVxPer],
                                             bool (&head)[kVxPer]) {
  if (i0 + kVxPer <= n) {
    const longlong2* p = reinterpret_cast<const longlong2*>(keys + i0);  // i0 is a multiple of 8, keys 16-B aligned
#pragma unroll
    for (int j = 0; j < kVxPer; j += 2) {
      const longlong2 q = p[j >> 1];
      k[j] = q.x;
      k[j + 1] = q.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kVxPer; ++j) k[j] = i0 + j < n ? keys[i0 + j] : 0;
  }
  int64_t prev = (i0 > 0 && i0 < n) ? keys[i0 - 1] : 0;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < kVxPer; ++j) {
    head[j] = i0 + j < n && (i0 + j == 0 || k[j] != prev);
    prev = k[j];
    cnt += head[j] ? 1 : 0;
  }
  return cnt;
}

__global__ __launch_bounds__(kVxThreads) void vx_tile_count_kernel(const int64_t* __restrict__ keys, int64_t n, int64_t ntiles,
                                                                   int32_t* __restrict__ tile_sum) {
  __shared__ int s_wave[kVxThreads / 64];
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int64_t k[kVxPer];
    bool head[kVxPer];
    const int cnt = vx_load_heads(keys, n, tile * kVxTile + (int64_t)threadIdx.x * kVxPer, k, head);
    int tot;
    block_excl_scan<kVxThreads>(cnt, s_wave, &tot);
    if (threadIdx.x == 0) tile_sum[tile] = tot;
    __syncthreads();  // s_wave is rewritten by the next trip
  }
}

// ONE workgroup: exclusive scan of the tile sums in place; summary[0] = M and the closing boundary offsets[M] = n
__global__ __launch_bounds__(kVxThreads) void vx_tile_scan_kernel(int32_t* __restrict__ tile_sum, int64_t ntiles, int64_t n,
                                                                  int32_t* __restrict__ summary,
                                                                  int64_t* __restrict__ csr_offsets) {
  __shared__ int s_wave[kVxThreads / 64];
  int carry = 0;
  for (int64_t base = 0; base < ntiles; base += kVxThreads) {
    const int64_t i = base + threadIdx.x;
    const int v = i < ntiles ? tile_sum[i] : 0;
    int tot;
    const int e = block_excl_scan<kVxThreads>(v, s_wave, &tot);
    if (i < ntiles) tile_sum[i] = carry + e;
    carry += tot;
    __syncthreads();  // s_wave is rewritten by the next trip
  }
  if (threadIdx.x == 0) {
    summary[0] = carry;
    csr_offsets[carry] = n;  // carry <= n: the caller's buffer holds n + 1 words
  }
}

__global__ __launch_bounds__(kVxThreads) void vx_apply_kernel(const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                                              int64_t n, int64_t ntiles, const int32_t* __restrict__ tile_sum,
                                                              int64_t* __restrict__ unique_keys,
                                                              int32_t* __restrict__ unique_coords,
                                                              int64_t* __restrict__ csr_offsets,
                                                              int64_t* __restrict__ to_orig, int64_t* __restrict__ to_unique) {
  __shared__ int s_wave[kVxThreads / 64];
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t i0 = tile * kVxTile + (int64_t)threadIdx.x * kVxPer;
    int64_t k[kVxPer];
    bool head[kVxPer];
    const int cnt = vx_load_heads(keys, n, i0, k, head);
    int tot;
    int64_t vid = (int64_t)tile_sum[tile] + block_excl_scan<kVxThreads>(cnt, s_wave, &tot) - 1;  // voxel of position i0 - 1
#pragma unroll
    for (int j = 0; j < kVxPer; ++j) {
      const int64_t i = i0 + j;
      if (i >= n) break;
      const int64_t row = perm[i];
      if (head[j]) {
        ++vid;
        if (vid >= 0 && vid < n) {
          csr_offsets[vid] = i;
          unique_keys[vid] = k[j];
          to_unique[vid] = row;  // stable sort: the first position of a run holds the run's smallest row
          if (unique_coords) {
            unique_coords[3 * vid] = (int32_t)(((k[j] >> 36) & kCoordMask) - kCoordBias);
            unique_coords[3 * vid + 1] = (int32_t)(((k[j] >> 18) & kCoordMask) - kCoordBias);
            unique_coords[3 * vid + 2] = (int32_t)((k[j] & kCoordMask) - kCoordBias);
          }
        }
      }
      if (row >= 0 && row < n) to_orig[row] = vid;
    }
    __syncthreads();  // s_wave is rewritten by the next trip
  }
}

// per voxel: the longest segment (integer atomic max) and, where the batch field of the key steps, the voxel offsets of the
// batch elements in between (every word written once: voxels are key-sorted, so the batch field ascends)
__global__ __launch_bounds__(kVxThreads) void vx_finish_kernel(const int64_t* __restrict__ unique_keys,
                                                               const int64_t* __restrict__ csr_offsets, int64_t n,
                                                               int32_t* __restrict__ summary,
                                                               int32_t* __restrict__ batch_voxel_offsets, int num_batches) {
  int64_t M = summary[0];
  if (M > n) M = n;
  int longest = 0;
  for (int64_t v = (int64_t)blockIdx.x * kVxThreads + threadIdx.x; v < M; v += (int64_t)gridDim.x * kVxThreads) {
    const int64_t len = csr_offsets[v + 1] - csr_offsets[v];
    longest = max(longest, (int)(len < INT_MAX ? len : INT_MAX));
    if (batch_voxel_offsets) {
      int b = (int)(unique_keys[v] >> 54);
      b = b < 0 ? 0 : (b > num_batches - 1 ? num_batches - 1 : b);
      const int before = v > 0 ? (int)(unique_keys[v - 1] >> 54) : -1;
      for (int q = max(before, -1) + 1; q <= b; ++q) batch_voxel_offsets[q] = (int32_t)v;
      if (v == M - 1)
        for (int q = b + 1; q <= num_batches; ++q) batch_voxel_offsets[q] = (int32_t)M;
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) longest = max(longest, __shfl_xor(longest, d));
  if ((threadIdx.x & 63) == 0 && longest > 0) atomicMax(summary + 1, longest);
}

// ---- element types ----------------------------------------------------------------------------------------------------------
template <int D> struct El;
template <> struct El<WCN_F32> {
  using S = float;
  static __device__ __forceinline__ float ld(S s) { return s; }
  static __device__ __forceinline__ S st(float f) { return f; }
};
template <> struct El<WCN_F16> {
  using S = uint16_t;
  static __device__ __forceinline__ float ld(S s) { return __half2float(__ushort_as_half(s)); }
  static __device__ __forceinline__ S st(float f) { return __half_as_ushort(__float2half(f)); }
};
template <> struct El<WCN_BF16> {
  using S = uint16_t;
  static __device__ __forceinline__ float ld(S s) { return __uint_as_float((uint32_t)s << 16); }
  static __device__ __forceinline__ S st(float f) { return __bfloat16_as_ushort(__float2bfloat16(f)); }
};

template <typename S, int V>
struct __attribute__((aligned(sizeof(S) * V))) Pack {
  S v[V];
};

template <int D, int V>
__device__ __forceinline__ void ld_pack(const typename El<D>::S* p, float (&f)[V]) {
  using S = typename El<D>::S;
  const Pack<S, V> q = *reinterpret_cast<const Pack<S, V>*>(p);
#pragma unroll
  for (int e = 0; e < V; ++e) f[e] = El<D>::ld(q.v[e]);
}

template <int D, int V>
__device__ __forceinline__ void st_pack(typename El<D>::S* p, const float (&f)[V]) {
  using S = typename El<D>::S;
  Pack<S, V> q;
#pragma unroll
  for (int e = 0; e < V; ++e) q.v[e] = El<D>::st(f[e]);
  *reinterpret_cast<Pack<S, V>*>(p) = q;
}

// ---- c. CSR gather-reduce ---------------------------------------------------------------------------------------------------
struct CgLong {  // the long segments and their chunks, listed per call
  int32_t* counters;   // [0] chunk items, [1] long segments
  int32_t* item_seg;   // [item_cap]
  int32_t* item_k;     // [item_cap] chunk number inside the segment
  int32_t* long_seg;   // [long_cap]
  int32_t* long_base;  // [long_cap] first item of the segment
  float* part;         // [item_cap][c]
  int64_t* part_arg;   // [item_cap][c] (max / min)
  int64_t item_cap, long_cap;
  size_t bytes;
};

static CgLong cg_carve(void* base, int64_t nnz, int64_t c, bool with_arg) {
  CgLong w;
  w.long_cap = nnz / kCgChunk + 1;  // a long segment holds more than kCgChunk rows
  w.item_cap = 2 * w.long_cap;      // ceil(len / chunk) <= len / chunk + 1 per long segment
  char* p = (char*)base;
  size_t at = 0;
  w.counters = (int32_t*)(p + at);
  at = align256(at + kCgCounterInts * 4);
  w.item_seg = (int32_t*)(p + at);
  at = align256(at + (size_t)w.item_cap * 4);
  w.item_k = (int32_t*)(p + at);
  at = align256(at + (size_t)w.item_cap * 4);
  w.long_seg = (int32_t*)(p + at);
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
template <int D, int V>
__device__ __forceinline__ void cg_rows(const typename El<D>::S* __restrict__ in, int64_t ld_in, int64_t n_in,
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
        ld_pack<D, V>(in + r[u] * ld_in + col, f[u]);
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
      ld_pack<D, V>(in + r * ld_in + col, f);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) f[e] = 0.f;
    }
    take(r, f);
  }
}

// L lanes (a power of two <= 64) own one list: ITEMS = false, a whole segment (longer ones are skipped when `split`);
// ITEMS = true, one chunk of a long segment into the fp32 partials.  Rows wider than L * V channels take several trips.
template <int D, int V, bool ITEMS>
__global__ __launch_bounds__(kVxThreads) void cg_reduce_kernel(const typename El<D>::S* __restrict__ in, int64_t ld_in,
                                                               int64_t n_in, const int64_t* __restrict__ indices,
                                                               const int64_t* __restrict__ offsets, int64_t m, int64_t nnz,
                                                               int c, int L, int op, int split,
                                                               typename El<D>::S* __restrict__ out, int64_t* __restrict__ arg,
                                                               CgLong w) {
  const int groups = kVxThreads / L;
  const int g = threadIdx.x / L, sub = threadIdx.x % L;
  int64_t total = m;
  if (ITEMS) {
    total = w.counters[0];
    if (total > w.item_cap) total = w.item_cap;
  }
  for (int64_t t = (int64_t)blockIdx.x * groups + g; t < total; t += (int64_t)gridDim.x * groups) {
    const int64_t seg = ITEMS ? w.item_seg[t] : t;
    if (seg < 0 || seg >= m) continue;
    int64_t j0 = offsets[seg], j1 = offsets[seg + 1];
    if (j0 < 0 || j1 > nnz || j1 < j0) j1 = j0 = 0;  // offsets that do not describe the list: an empty segment
    const int64_t len = j1 - j0;
    if (ITEMS) {
      j0 += (int64_t)w.item_k[t] * kCgChunk;
      if (j0 > j1) j0 = j1;
      if (j1 - j0 > kCgChunk) j1 = j0 + kCgChunk;
    } else if (split && len > kCgChunk) {
      continue;
    }
    for (int col = sub * V; col < c; col += L * V) {
      float acc[V];
      int64_t best[V];
#pragma unroll
      for (int e = 0; e < V; ++e) { acc[e] = 0.f; best[e] = -1; }
      cg_rows<D, V>(in, ld_in, n_in, indices, j0, j1, col, op, acc, best);
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
        st_pack<D, V>(out + seg * c + col, acc);
        if (arg) {
#pragma unroll
          for (int e = 0; e < V; ++e) arg[seg * c + col + e] = best[e];
        }
      }
    }
  }
}

// one wave looks at 64 segments; every long one takes its run of items with one integer atomic and the wave writes the run
__global__ __launch_bounds__(kVxThreads) void cg_collect_kernel(const int64_t* __restrict__ offsets, int64_t m, int64_t nnz,
                                                                CgLong w) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (kVxThreads / 64) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (kVxThreads / 64);
  for (int64_t base = wave * 64; base < m; base += nwaves * 64) {
    const int64_t seg = base + lane;
    int nch = 0;
    if (seg < m) {
      const int64_t j0 = offsets[seg], j1 = offsets[seg + 1];
      if (j0 >= 0 && j1 <= nnz && j1 - j0 > kCgChunk) nch = (int)((j1 - j0 + kCgChunk - 1) / kCgChunk);
    }
    unsigned long long todo = __ballot(nch > 0);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int s_seg = (int)__shfl((int)seg, src), s_n = __shfl(nch, src);
      int first = 0, slot = 0;
      if (lane == 0) {
        first = atomicAdd(w.counters, s_n);
        slot = atomicAdd(w.counters + 1, 1);
        if (slot < w.long_cap) {
          w.long_seg[slot] = s_seg;
          w.long_base[slot] = first;
        }
      }
      first = __shfl(first, 0);
      for (int k = lane; k < s_n; k += 64) {
        if ((int64_t)first + k < w.item_cap) {
          w.item_seg[first + k] = s_seg;
          w.item_k[first + k] = k;
        }
      }
    }
  }
}

// L lanes per long segment: its partials in chunk order
template <int D>
__global__ __launch_bounds__(kVxThreads) void cg_combine_kernel(const int64_t* __restrict__ offsets, int64_t m, int c, int L,
                                                                int op, typename El<D>::S* __restrict__ out,
                                                                int64_t* __restrict__ arg, CgLong w) {
  const int groups = kVxThreads / L;
  const int g = threadIdx.x / L, sub = threadIdx.x % L;
  int64_t total = w.counters[1];
  if (total > w.long_cap) total = w.long_cap;
  for (int64_t t = (int64_t)blockIdx.x * groups + g; t < total; t += (int64_t)gridDim.x * groups) {
    const int64_t seg = w.long_seg[t], first = w.long_base[t];
    if (seg < 0 || seg >= m) continue;
    const int64_t len = offsets[seg + 1] - offsets[seg];
    const int64_t nch = (len + kCgChunk - 1) / kCgChunk;
    if (first < 0 || first + nch > w.item_cap) continue;
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
      out[seg * c + col] = El<D>::st(acc);
      if (arg) arg[seg * c + col] = best;
    }
  }
}

static int pow2_lanes(int64_t pieces) {
  int L = 1;
  while (L < pieces && L < 64) L <<= 1;
  return L;
}


template <int D, int V>
static void cg_launch(const void* in, int64_t ld_in, int64_t n_in, const int64_t* indices, const int64_t* offsets, int64_t m,
                      int64_t nnz, int c, int op, bool split, void* out, int64_t* arg, const CgLong& w, hipStream_t s) {
  using S = typename El<D>::S;
  const int L = pow2_lanes(ceil_div(c, V)), groups = kVxThreads / L;
  hipLaunchKernelGGL((cg_reduce_kernel<D, V, false>), dim3(vx_grid(ceil_div(m, groups))), dim3(kVxThreads), 0, s, (const S*)in,
                     ld_in, n_in, indices, offsets, m, nnz, c, L, op, split ? 1 : 0, (S*)out, arg, w);
  if (!split) return;
  hipLaunchKernelGGL(cg_collect_kernel, dim3(vx_grid(ceil_div(m, kVxThreads))), dim3(kVxThreads), 0, s, offsets, m, nnz, w);
  hipLaunchKernelGGL((cg_reduce_kernel<D, V, true>), dim3(vx_grid(ceil_div(w.item_cap, groups))), dim3(kVxThreads), 0, s,
                     (const S*)in, ld_in, n_in, indices, offsets, m, nnz, c, L, op, 1, (S*)out, arg, w);
  const int Lc = pow2_lanes(c);
  hipLaunchKernelGGL(cg_combine_kernel<D>, dim3(vx_grid(ceil_div(w.long_cap, kVxThreads / Lc))), dim3(kVxThreads), 0, s,
                     offsets, m, c, Lc, op, (S*)out, arg, w);
}

// widest piece (elements per lane) that the channel count, the row strides and the pointers allow: 16 B, 8 B or one element
static int piece_elems(int dtype, int64_t c, int64_t c2, int64_t ld_a, int64_t ld_b, const void* p0, const void* p1,
                       const void* p2) {
  const int es = dtype == WCN_F32 ? 4 : 2;
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
template <int D, int V>
__global__ __launch_bounds__(kVxThreads) void row_spread_kernel(const typename El<D>::S* __restrict__ src,
                                                                const int64_t* __restrict__ to_orig, int64_t n, int64_t m,
                                                                int c, const typename El<D>::S* __restrict__ skip, int cs,
                                                                int64_t ld_out, int mode, const int64_t* __restrict__ offsets,
                                                                const int64_t* __restrict__ arg,
                                                                typename El<D>::S* __restrict__ out) {
  const int pc = c / V, pw = pc + cs / V;
  const int64_t total = n * pw;
  for (int64_t e = (int64_t)blockIdx.x * kVxThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kVxThreads) {
    const int64_t i = e / pw;
    const int p = (int)(e - i * pw);
    float f[V];
    if (p >= pc) {
      const int col = (p - pc) * V;
      ld_pack<D, V>(skip + i * cs + col, f);
      st_pack<D, V>(out + i * ld_out + c + col, f);
      continue;
    }
    const int col = p * V;
    const int64_t v = to_orig[i];
    if (v < 0 || v >= m) {
#pragma unroll
      for (int q = 0; q < V; ++q) f[q] = 0.f;
    } else {
      ld_pack<D, V>(src + v * c + col, f);
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
    st_pack<D, V>(out + i * ld_out + col, f);
  }
}

template <int D, int V>
static void spread_launch(const void* src, const int64_t* to_orig, int64_t n, int64_t m, int c, const void* skip, int cs,
                          int64_t ld_out, int mode, const int64_t* offsets, const int64_t* arg, void* out, hipStream_t s) {
  using S = typename El<D>::S;
  const int64_t pieces = n * (int64_t)((c + cs) / V);
  hipLaunchKernelGGL((row_spread_kernel<D, V>), dim3(vx_grid(ceil_div(pieces, kVxThreads))), dim3(kVxThreads), 0, s,
                     (const S*)src, to_orig, n, m, c, (const S*)skip, cs, ld_out, mode, offsets, arg, (S*)out);
}

}  // namespace wcn

using namespace wcn;

#define WCN_VX_DISPATCH(FN, dtype, v, ...)                                              \
  do {                                                                                  \
    if (dtype == WCN_F32) {                                                             \
      if (v == 4) FN<WCN_F32, 4>(__VA_ARGS__);                                          \
      else if (v == 2) FN<WCN_F32, 2>(__VA_ARGS__);                                     \
      else FN<WCN_F32, 1>(__VA_ARGS__);                                                 \
    } else if (dtype == WCN_F16) {                                                      \
      if (v == 8) FN<WCN_F16, 8>(__VA_ARGS__);                                          \
      else if (v == 4) FN<WCN_F16, 4>(__VA_ARGS__);                                     \
      else FN<WCN_F16, 1>(__VA_ARGS__);                                                 \
    } else {                                                                            \
      if (v == 8) FN<WCN_BF16, 8>(__VA_ARGS__);                                         \
      else if (v == 4) FN<WCN_BF16, 4>(__VA_ARGS__);                                    \
      else FN<WCN_BF16, 1>(__VA_ARGS__);                                                \
    }                                                                                   \
  } while (0)

extern "C" {

int32_t wcn_csr_chunk_rows(void) { return kCgChunk; }

int wcn_voxel_keys(const float* points, int64_t n, const int32_t* batch_offsets, int32_t num_batches, float inv_voxel_size,
                   int64_t* keys, int32_t* status, wcn_stream_t stream) {
  if (n < 0 || n > INT32_MAX || !status) return WCN_ERROR_INVALID_PARAMETERS;
  if (points && (num_batches < 1 || num_batches > kBatchMax + 1 || !(inv_voxel_size > 0.f) || !(inv_voxel_size < FLT_MAX)))
    return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, 4, s) != hipSuccess) return WCN_ERROR_KERNEL_EXECUTION;
  if (n == 0 || !points) return WCN_SUCCESS;  // null points: the keys are the caller's own codes
  if (!batch_offsets || !keys) return WCN_ERROR_INVALID_PARAMETERS;
  hipLaunchKernelGGL(vx_keys_kernel, dim3(vx_grid(ceil_div(n, kVxThreads))), dim3(kVxThreads), 0, s, points, n, batch_offsets,
                     (int)num_batches, inv_voxel_size, keys, status);
  return launch_status();
}

size_t wcn_voxel_map_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return align256((size_t)ceil_div(n > 0 ? n : 1, kVxTile) * 4);
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
  const int64_t ntiles = ceil_div(n, kVxTile);
  int32_t* tile_sum = (int32_t*)workspace;
  const dim3 block(kVxThreads), tiles(vx_grid(ntiles));
  hipLaunchKernelGGL(vx_tile_count_kernel, tiles, block, 0, s, sorted_keys, n, ntiles, tile_sum);
  hipLaunchKernelGGL(vx_tile_scan_kernel, dim3(1), block, 0, s, tile_sum, ntiles, n, summary, csr_offsets);
  hipLaunchKernelGGL(vx_apply_kernel, tiles, block, 0, s, sorted_keys, perm, n, ntiles, tile_sum, unique_keys, unique_coords,
                     csr_offsets, to_orig, to_unique);
  hipLaunchKernelGGL(vx_finish_kernel, dim3(vx_grid(ceil_div(n, kVxThreads))), block, 0, s, unique_keys, csr_offsets, n,
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
  const bool split = max_segment < 0 || max_segment > kCgChunk;  // < 0: the caller does not know the longest segment
  CgLong w{};
  hipStream_t s = (hipStream_t)stream;
  if (split) {
    if (!workspace || !aligned_to(workspace, 16)) return WCN_ERROR_INVALID_PARAMETERS;
    w = cg_carve(workspace, nnz, c, op >= kOpMax);
    if (workspace_bytes < w.bytes) return WCN_ERROR_INVALID_PARAMETERS;
    if (hipMemsetAsync(w.counters, 0, kCgCounterInts * 4, s) != hipSuccess) return WCN_ERROR_KERNEL_EXECUTION;
  }
  const int v = piece_elems(dtype, c, 0, ld_in, 0, in, out, nullptr);
  WCN_VX_DISPATCH(cg_launch, dtype, v, in, ld_in, n_in, indices, offsets, m, nnz, (int)c, (int)op, split, out, arg, w, s);
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
  WCN_VX_DISPATCH(spread_launch, dtype, v, src, to_orig, n, m, (int)c, skip, (int)cs, ld_out, (int)mode, offsets, arg, out,
                  (hipStream_t)stream);
  return launch_status();
}

}  // extern "C"
