// window_group.hip - voxels grouped into 3-D windows by a counting sort: the step that turns coordinates into the attention
// sequences of SpaceAttention (reference: warpconvnet/csrc/window_grouping_kernels.cu, driven by
// nn/functional/voxel_encode.py:237-316).
//
// One call = seven launches on one stream, no host read in between:
//   1. wg_code_kernel         window code of every voxel + dense histogram (integer atomics)
//   2. wg_tile_reduce_kernel  per 2048-bin tile: voxels, non-empty bins, largest bin
//   3. wg_tile_scan_kernel    ONE workgroup scans the tile sums; writes the summary (S, max_count) and cu_seqlens[S]
//   4. wg_apply_kernel        per tile again: histogram -> exclusive offsets in place; non-empty bins -> cu_seqlens / counts
//   5. wg_scatter_kernel      every voxel takes a slot of its window's segment (integer atomic on the offset word)
//   6. wg_sort_wave_kernel    segments of <= 64 rows: one wave each, rank by counting through lane shuffles
//   7. wg_sort_block_kernel   segments of 65 .. kWgSegMax rows: one workgroup each, in LDS (rank by counting up to
//                             kWgRankMax rows, bitonic network above); both write perm and inverse_perm
// 2-4 are the block-sums / scan-of-sums / apply pattern: no kernel waits on another workgroup.  The slot a voxel takes in
// step 5 depends on the order the atomics retire, but the SET of rows of a segment does not; sorting the segment ascending
// makes perm the stable sort by code, the same bits in every run.  Segments longer than kWgSegMax are left unwritten: the
// caller sees max_count in the summary and takes another path.  Every grid is capped at kRowMaxGrid workgroups (row_lists.h)
// and strides.
#include <limits.h>

#include "row_lists.h"

namespace wcn {

constexpr int kWgThreads = 256;
constexpr int kWgPer = 8;
constexpr int kWgTile = kWgThreads * kWgPer;  // bins of one scan tile
constexpr int kWgSegMax = 8192;               // rows of the longest segment sorted in LDS (32 KiB of the 160 KiB)
constexpr int kWgRankMax = 1024;              // up to here a segment is ranked by counting, above by a bitonic network
constexpr int kWgFlagInts = 64;               // the error word and its padding, behind the histogram (one memset)

struct I3 {
  int x, y, z;
};

struct WgCarve {
  int32_t* hist;      // [padded bins] counts, then exclusive offsets, then (after the scatter) end offsets
  int32_t* flag;      // != 0: a voxel fell outside the announced grid
  int32_t* tile_sum;  // [ntiles]
  int32_t* tile_nz;   // [ntiles]
  int32_t* tile_max;  // [ntiles]
  int32_t* slots;     // [n] rows in window order, unordered inside a window
  int64_t ntiles;
  size_t bytes;
};

static WgCarve wg_carve(void* base, int64_t n, int64_t num_bins) {
  WgCarve c;
  c.ntiles = ceil_div(num_bins > 0 ? num_bins : 1, kWgTile);
  char* p = (char*)base;
  size_t at = 0;
  c.hist = (int32_t*)(p + at);
  at += (size_t)c.ntiles * kWgTile * 4;
  c.flag = (int32_t*)(p + at);
  at = align256(at + kWgFlagInts * 4);
  c.tile_sum = (int32_t*)(p + at);
  at = align256(at + (size_t)c.ntiles * 4);
  c.tile_nz = (int32_t*)(p + at);
  at = align256(at + (size_t)c.ntiles * 4);
  c.tile_max = (int32_t*)(p + at);
  at = align256(at + (size_t)c.ntiles * 4);
  c.slots = (int32_t*)(p + at);
  at = align256(at + (size_t)(n > 0 ? n : 0) * 4);
  c.bytes = at;
  return c;
}

// code = b * W + (wx * gs.y + wy) * gs.z + wz with w = (coord + shift - lo) / window (window_group_histogram_kernel of the
// reference); the batch element by bisection of batch_offsets, empty elements are legal.  A voxel outside the announced
// box raises the flag instead of indexing past the histogram.
__global__ __launch_bounds__(kWgThreads) void wg_code_kernel(const int32_t* __restrict__ coords, int64_t n,
                                                             const int32_t* __restrict__ batch_offsets, int num_batches,
                                                             I3 window, I3 shift, I3 lo, I3 gs, int64_t W,
                                                             int64_t* __restrict__ codes, int32_t* __restrict__ hist,
                                                             int32_t* __restrict__ flag) {
  for (int64_t i = (int64_t)blockIdx.x * kWgThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kWgThreads) {
    int b = 0, hi = num_batches;
    while (b < hi) {
      const int mid = (b + hi) >> 1;
      if (i < batch_offsets[mid + 1]) hi = mid; else b = mid + 1;
    }
    const int64_t dx = (int64_t)coords[3 * i] + shift.x - lo.x;
    const int64_t dy = (int64_t)coords[3 * i + 1] + shift.y - lo.y;
    const int64_t dz = (int64_t)coords[3 * i + 2] + shift.z - lo.z;
    const int64_t wx = dx / window.x, wy = dy / window.y, wz = dz / window.z;
    const bool ok = b < num_batches && dx >= 0 && dy >= 0 && dz >= 0 && wx < gs.x && wy < gs.y && wz < gs.z;
    if (!ok) {
      codes[i] = -1;
      atomicOr(flag, 1);
      continue;
    }
    const int64_t code = (int64_t)b * W + (wx * gs.y + wy) * gs.z + wz;
    codes[i] = code;
    atomicAdd(hist + code, 1);
  }
}

__device__ __forceinline__ void wg_load_tile(const int32_t* __restrict__ hist, int64_t tile, int (&v)[kWgPer]) {
  const int4* p = reinterpret_cast<const int4*>(hist + tile * kWgTile + (int64_t)threadIdx.x * kWgPer);
#pragma unroll
  for (int j = 0; j < kWgPer; j += 4) {
    const int4 q = p[j >> 2];
    v[j] = q.x; v[j + 1] = q.y; v[j + 2] = q.z; v[j + 3] = q.w;
  }
}

__global__ __launch_bounds__(kWgThreads) void wg_tile_reduce_kernel(const int32_t* __restrict__ hist, int64_t ntiles,
                                                                    int32_t* __restrict__ tile_sum,
                                                                    int32_t* __restrict__ tile_nz,
                                                                    int32_t* __restrict__ tile_max) {
  __shared__ int s_part[3][kWgThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int v[kWgPer];
    wg_load_tile(hist, tile, v);
    int sum = 0, nz = 0, mx = 0;
#pragma unroll
    for (int j = 0; j < kWgPer; ++j) {
      sum += v[j];
      nz += v[j] > 0 ? 1 : 0;
      mx = max(mx, v[j]);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      sum += __shfl_xor(sum, d);
      nz += __shfl_xor(nz, d);
      mx = max(mx, __shfl_xor(mx, d));
    }
    if (lane == 0) {
      s_part[0][wave] = sum;
      s_part[1][wave] = nz;
      s_part[2][wave] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int a = 0, z = 0, m = 0;
#pragma unroll
      for (int w = 0; w < kWgThreads / 64; ++w) {
        a += s_part[0][w];
        z += s_part[1][w];
        m = max(m, s_part[2][w]);
      }
      tile_sum[tile] = a;
      tile_nz[tile] = z;
      tile_max[tile] = m;
    }
    __syncthreads();  // s_part is rewritten by the next trip
  }
}

// ONE workgroup: exclusive scans of tile_sum and tile_nz in place, 256 tiles a trip with a carry; the summary and the closing
// boundary cu_seqlens[S] = number of voxels.  S = -1 reports the raised flag.
__global__ __launch_bounds__(kWgThreads) void wg_tile_scan_kernel(int32_t* __restrict__ tile_sum, int32_t* __restrict__ tile_nz,
                                                                  const int32_t* __restrict__ tile_max, int64_t ntiles,
                                                                  const int32_t* __restrict__ flag,
                                                                  int32_t* __restrict__ summary,
                                                                  int32_t* __restrict__ cu_seqlens, int64_t seg_capacity) {
  __shared__ int s_a[kWgThreads / 64], s_z[kWgThreads / 64], s_m[kWgThreads / 64];
  int carry_a = 0, carry_z = 0, mx = 0;
  for (int64_t base = 0; base < ntiles; base += kWgThreads) {
    const int64_t i = base + threadIdx.x;
    const int a = i < ntiles ? tile_sum[i] : 0, z = i < ntiles ? tile_nz[i] : 0;
    if (i < ntiles) mx = max(mx, tile_max[i]);
    int tot_a, tot_z;
    const int ea = block_excl_scan<kWgThreads>(a, s_a, &tot_a);
    const int ez = block_excl_scan<kWgThreads>(z, s_z, &tot_z);
    if (i < ntiles) {
      tile_sum[i] = carry_a + ea;
      tile_nz[i] = carry_z + ez;
    }
    carry_a += tot_a;
    carry_z += tot_z;
    __syncthreads();  // s_a / s_z are rewritten by the next trip
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mx = max(mx, __shfl_xor(mx, d));
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    int m = 0;
#pragma unroll
    for (int w = 0; w < kWgThreads / 64; ++w) m = max(m, s_m[w]);
    const bool bad = flag[0] != 0;
    summary[0] = bad ? -1 : carry_z;
    summary[1] = bad ? 0 : m;
    if (!bad && carry_z <= seg_capacity) cu_seqlens[carry_z] = carry_a;
  }
}

__global__ __launch_bounds__(kWgThreads) void wg_apply_kernel(int32_t* __restrict__ hist, int64_t ntiles,
                                                              const int32_t* __restrict__ tile_sum,
                                                              const int32_t* __restrict__ tile_nz,
                                                              int32_t* __restrict__ cu_seqlens, int64_t* __restrict__ counts,
                                                              int64_t seg_capacity) {
  __shared__ int s_a[kWgThreads / 64], s_z[kWgThreads / 64];
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int v[kWgPer];
    wg_load_tile(hist, tile, v);
    int sum = 0, nz = 0;
#pragma unroll
    for (int j = 0; j < kWgPer; ++j) {
      sum += v[j];
      nz += v[j] > 0 ? 1 : 0;
    }
    int tot;
    int run = tile_sum[tile] + block_excl_scan<kWgThreads>(sum, s_a, &tot);
    int64_t seg = (int64_t)tile_nz[tile] + block_excl_scan<kWgThreads>(nz, s_z, &tot);
    int o[kWgPer];
#pragma unroll
    for (int j = 0; j < kWgPer; ++j) {
      o[j] = run;
      if (v[j] > 0) {
        if (seg < seg_capacity) {
          cu_seqlens[seg] = run;
          counts[seg] = v[j];
        }
        ++seg;
      }
      run += v[j];
    }
    int4* p = reinterpret_cast<int4*>(hist + tile * kWgTile + (int64_t)threadIdx.x * kWgPer);
#pragma unroll
    for (int j = 0; j < kWgPer; j += 4) p[j >> 2] = make_int4(o[j], o[j + 1], o[j + 2], o[j + 3]);
    __syncthreads();  // s_a / s_z are rewritten by the next trip
  }
}

__global__ __launch_bounds__(kWgThreads) void wg_scatter_kernel(const int64_t* __restrict__ codes, int64_t n,
                                                                int32_t* __restrict__ offs, int32_t* __restrict__ slots,
                                                                const int32_t* __restrict__ flag) {
  if (flag[0] != 0) return;
  for (int64_t i = (int64_t)blockIdx.x * kWgThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kWgThreads) {
    const int64_t code = codes[i];
    if (code < 0) continue;
    const int pos = atomicAdd(offs + code, 1);
    if (pos >= 0 && pos < n) slots[pos] = (int32_t)i;
  }
}

__device__ __forceinline__ void wg_emit(int64_t* __restrict__ perm, int64_t* __restrict__ inverse_perm, int64_t n,
                                        int64_t pos, int32_t row) {
  perm[pos] = row;
  if (row >= 0 && row < n) inverse_perm[row] = pos;
}

// one wave per segment of <= 64 rows: rank of a row = rows of the segment below it
__global__ __launch_bounds__(kWgThreads) void wg_sort_wave_kernel(const int32_t* __restrict__ slots,
                                                                  const int32_t* __restrict__ cu_seqlens,
                                                                  const int32_t* __restrict__ summary, int64_t n,
                                                                  int64_t* __restrict__ perm,
                                                                  int64_t* __restrict__ inverse_perm) {
  const int64_t S = summary[0];
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (kWgThreads / 64);
  for (int64_t s = (int64_t)blockIdx.x * (kWgThreads / 64) + (threadIdx.x >> 6); s < S; s += nwaves) {
    const int beg = cu_seqlens[s], len = cu_seqlens[s + 1] - beg;
    if (len <= 0 || len > 64 || beg < 0 || (int64_t)beg + len > n) continue;  // wave-uniform
    const int32_t v = lane < len ? slots[beg + lane] : INT_MAX;
    int rank = 0;
    for (int j = 0; j < len; ++j) rank += __shfl(v, j) < v ? 1 : 0;
    if (lane < len) wg_emit(perm, inverse_perm, n, (int64_t)beg + rank, v);
  }
}

// one workgroup per segment of 65 .. kWgSegMax rows, the segment in LDS
__global__ __launch_bounds__(kWgThreads) void wg_sort_block_kernel(const int32_t* __restrict__ slots,
                                                                   const int32_t* __restrict__ cu_seqlens,
                                                                   const int32_t* __restrict__ summary, int64_t n,
                                                                   int64_t* __restrict__ perm,
                                                                   int64_t* __restrict__ inverse_perm) {
  __shared__ int32_t sh[kWgSegMax];
  const int64_t S = summary[0];
  for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
    const int beg = cu_seqlens[s], len = cu_seqlens[s + 1] - beg;
    if (len <= 64 || len > kWgSegMax || beg < 0 || (int64_t)beg + len > n) continue;  // workgroup-uniform
    if (len <= kWgRankMax) {
      for (int t = threadIdx.x; t < len; t += kWgThreads) sh[t] = slots[beg + t];
      __syncthreads();
      for (int t = threadIdx.x; t < len; t += kWgThreads) {
        const int32_t v = sh[t];
        int rank = 0;
        for (int j = 0; j < len; ++j) rank += sh[j] < v ? 1 : 0;  // every lane reads one address: a broadcast
        wg_emit(perm, inverse_perm, n, (int64_t)beg + rank, v);
      }
    } else {
      int P = kWgRankMax;
      while (P < len) P <<= 1;  // <= kWgSegMax
      for (int t = threadIdx.x; t < P; t += kWgThreads) sh[t] = t < len ? slots[beg + t] : INT_MAX;
      __syncthreads();
      for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int t = threadIdx.x; t < P; t += kWgThreads) {
            const int u = t ^ j;
            if (u > t) {
              const int32_t a = sh[t], b = sh[u];
              if ((a > b) == ((t & k) == 0)) {
                sh[t] = b;
                sh[u] = a;
              }
            }
          }
          __syncthreads();
        }
      }
      for (int t = threadIdx.x; t < len; t += kWgThreads) wg_emit(perm, inverse_perm, n, (int64_t)beg + t, sh[t]);
    }
    __syncthreads();  // sh is rewritten by the next trip
  }
}

}  // namespace wcn

using namespace wcn;

extern "C" {

int32_t wcn_window_group_max_segment(void) { return kWgSegMax; }

size_t wcn_window_group_workspace_bytes(int64_t n, int64_t num_bins) {
  if (n < 0 || num_bins < 0) return 0;
  return wg_carve(nullptr, n, num_bins).bytes;
}

int wcn_window_group(const int32_t* coords, int64_t n, const int32_t* batch_offsets, int32_t num_batches,
                     const int32_t window[3], const int32_t shift[3], const int32_t min_coord[3], const int32_t grid_shape[3],
                     int64_t* codes, int64_t* perm, int64_t* inverse_perm, int32_t* cu_seqlens, int64_t* counts,
                     int32_t* summary, void* workspace, size_t workspace_bytes, wcn_stream_t stream) {
  if (n < 0 || n > INT32_MAX || num_batches < 1 || !window || !shift || !min_coord || !grid_shape || !summary || !cu_seqlens)
    return WCN_ERROR_INVALID_PARAMETERS;
  int64_t W = 1;
  for (int a = 0; a < 3; ++a) {
    if (window[a] < 1 || grid_shape[a] < 1) return WCN_ERROR_INVALID_PARAMETERS;
    W *= grid_shape[a];
    if (W > INT32_MAX) return WCN_ERROR_INVALID_PARAMETERS;
  }
  const int64_t num_bins = W * num_batches;
  if (num_bins > INT32_MAX - kWgTile) return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {  // no voxel: no window
    if (hipMemsetAsync(summary, 0, 8, s) != hipSuccess || hipMemsetAsync(cu_seqlens, 0, 4, s) != hipSuccess)
      return WCN_ERROR_KERNEL_EXECUTION;
    return WCN_SUCCESS;
  }
  if (!coords || !batch_offsets || !codes || !perm || !inverse_perm || !counts || !workspace ||
      !aligned_to(workspace, 16))
    return WCN_ERROR_INVALID_PARAMETERS;
  const WgCarve c = wg_carve(workspace, n, num_bins);
  if (workspace_bytes < c.bytes) return WCN_ERROR_INVALID_PARAMETERS;
  const int64_t seg_capacity = n < num_bins ? n : num_bins;  // cu_seqlens holds seg_capacity + 1 words, counts seg_capacity
  if (hipMemsetAsync(c.hist, 0, ((size_t)c.ntiles * kWgTile + kWgFlagInts) * 4, s) != hipSuccess)
    return WCN_ERROR_KERNEL_EXECUTION;
  const I3 win{window[0], window[1], window[2]}, sh{shift[0], shift[1], shift[2]};
  const I3 lo{min_coord[0], min_coord[1], min_coord[2]}, gs{grid_shape[0], grid_shape[1], grid_shape[2]};
  const dim3 block(kWgThreads);
  const dim3 rows(capped_grid(ceil_div(n, kWgThreads))), tiles(capped_grid(c.ntiles));
  hipLaunchKernelGGL(wg_code_kernel, rows, block, 0, s, coords, n, batch_offsets, (int)num_batches, win, sh, lo, gs, W, codes,
                     c.hist, c.flag);
  hipLaunchKernelGGL(wg_tile_reduce_kernel, tiles, block, 0, s, c.hist, c.ntiles, c.tile_sum, c.tile_nz, c.tile_max);
  hipLaunchKernelGGL(wg_tile_scan_kernel, dim3(1), block, 0, s, c.tile_sum, c.tile_nz, c.tile_max, c.ntiles, c.flag, summary,
                     cu_seqlens, seg_capacity);
  hipLaunchKernelGGL(wg_apply_kernel, tiles, block, 0, s, c.hist, c.ntiles, c.tile_sum, c.tile_nz, cu_seqlens, counts,
                     seg_capacity);
  hipLaunchKernelGGL(wg_scatter_kernel, rows, block, 0, s, codes, n, c.hist, c.slots, c.flag);
  hipLaunchKernelGGL(wg_sort_wave_kernel, dim3(capped_grid(ceil_div(seg_capacity, kWgThreads / 64))), block, 0, s, c.slots,
                     cu_seqlens, summary, n, perm, inverse_perm);
  hipLaunchKernelGGL(wg_sort_block_kernel, dim3(capped_grid(seg_capacity)), block, 0, s, c.slots, cu_seqlens, summary, n, perm,
                     inverse_perm);
  return launch_status();
}

}  // extern "C"
