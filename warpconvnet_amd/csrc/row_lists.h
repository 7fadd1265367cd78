// row_lists.h - the map and segment layer under voxelize.hip and lattice.hip, with the launch constants that grid.hip and
// window_group.hip share with them.  Every kernel here is a template (the ones without a parameter of their own over an
// unused int), so that a file carries only the kernels it launches.
//
//   a. launch      one workgroup size, one grid cap, one lanes-per-row rule
//   b. runs -> map sorted keys + permutation -> CSR offsets by run, the run of every position, the longest row.  Run heads are
//                  counted per kRunTile-key tile, ONE workgroup scans the tile sums, the tiles are applied: no kernel waits on
//                  another workgroup.  What a key is comes from a key policy, what a run head and a position write from a writer.
//   c. long rows   the chunk rule: a row of more than kRowChunk entries is cut into chunks of kRowChunk, each summed
//                  by its own lane group into a partial, and the partials are added in chunk order.  The list of long rows and
//                  their chunks is built here; where it lives and what a chunk sums is the including file's.
// The integer atomics (longest row, the list's two counters) give the same result in any order.
#pragma once

#include <limits.h>

#include "wcn_common.h"

namespace wcn {

// ---- a. launch --------------------------------------------------------------------------------------------------------------
constexpr int kRowThreads = 256;                   // threads of a workgroup
constexpr int kRunPer = 8;                         // sorted keys per thread of a run tile
constexpr int kRunTile = kRowThreads * kRunPer;    // sorted keys of one scan tile
constexpr int kRowMaxGrid = 4096;                  // every grid is capped here and strides
constexpr int kRowChunk = 256;                     // entries of one chunk of a long row (the chunk rule)
constexpr int kRowListCounterInts = 64;            // list header: [0] chunk items, [1] long rows; padded to 256 B

inline unsigned capped_grid(int64_t items) {
  const int64_t g = items < 1 ? 1 : items;
  return (unsigned)(g < kRowMaxGrid ? g : kRowMaxGrid);
}

// lanes of one row of `pieces` accesses: the power of two that covers them, 64 at the most
inline int row_lanes(int64_t pieces) {
  int L = 1;
  while (L < pieces && L < 64) L <<= 1;
  return L;
}

// ---- b. runs -> map ---------------------------------------------------------------------------------------------------------
// A key policy `Keys` has a type Key (Key{} = any value), load(n, i0, k): the kRunPer keys from sorted position i0 on (past n:
// any value), at(i): key i, and differ(a, b).  Thread t of a tile owns the sorted positions tile * kRunTile + t * kRunPer ..
// + kRunPer - 1; head = first position of a run.
template <typename Keys>
__device__ __forceinline__ int load_heads(const Keys& keys, int64_t n, int64_t i0, typename Keys::Key (&k)[kRunPer],
                                          bool (&head)[kRunPer]) {
  keys.load(n, i0, k);
  typename Keys::Key prev = typename Keys::Key{};
  if (i0 > 0 && i0 < n) prev = keys.at(i0 - 1);
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < kRunPer; ++j) {
    head[j] = i0 + j < n && (i0 + j == 0 || Keys::differ(k[j], prev));
    prev = k[j];
    cnt += head[j] ? 1 : 0;
  }
  return cnt;
}

template <typename Keys>
__global__ __launch_bounds__(kRowThreads) void run_count_kernel(Keys keys, int64_t n, int64_t ntiles,
                                                                int32_t* __restrict__ tile_sum) {
  __shared__ int s_wave[kRowThreads / 64];
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    typename Keys::Key k[kRunPer];
    bool head[kRunPer];
    const int cnt = load_heads(keys, n, tile * kRunTile + (int64_t)threadIdx.x * kRunPer, k, head);
    int tot;
    block_excl_scan<kRowThreads>(cnt, s_wave, &tot);
    if (threadIdx.x == 0) tile_sum[tile] = tot;
    __syncthreads();  // s_wave is rewritten by the next trip
  }
}

// ONE workgroup: exclusive scan of the tile sums in place; summary[0] = runs and the closing boundary offsets[runs] = n
template <int = 0>
__global__ __launch_bounds__(kRowThreads) void run_scan_kernel(int32_t* __restrict__ tile_sum, int64_t ntiles, int64_t n,
                                                               int32_t* __restrict__ summary,
                                                               int64_t* __restrict__ offsets) {
  __shared__ int s_wave[kRowThreads / 64];
  int carry = 0;
  for (int64_t base = 0; base < ntiles; base += kRowThreads) {
    const int64_t i = base + threadIdx.x;
    const int v = i < ntiles ? tile_sum[i] : 0;
    int tot;
    const int e = block_excl_scan<kRowThreads>(v, s_wave, &tot);
    if (i < ntiles) tile_sum[i] = carry + e;
    carry += tot;
    __syncthreads();  // s_wave is rewritten by the next trip
  }
  if (threadIdx.x == 0) {
    summary[0] = carry;
    offsets[carry] = n;  // carry <= n: the caller's buffer holds n + 1 words
  }
}

// offsets[run] = its first position; a writer `out` has head(run, row, key) for the first position of a run (row = perm there:
// under a stable sort the run's smallest) and each(row, run) for every position whose row lies in [0, n)
template <typename Keys, typename Writer>
__global__ __launch_bounds__(kRowThreads) void run_apply_kernel(Keys keys, const int64_t* __restrict__ perm, int64_t n,
                                                                int64_t ntiles, const int32_t* __restrict__ tile_sum,
                                                                int64_t* __restrict__ offsets, Writer out) {
  __shared__ int s_wave[kRowThreads / 64];
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t i0 = tile * kRunTile + (int64_t)threadIdx.x * kRunPer;
    typename Keys::Key k[kRunPer];
    bool head[kRunPer];
    const int cnt = load_heads(keys, n, i0, k, head);
    int tot;
    int64_t run = (int64_t)tile_sum[tile] + block_excl_scan<kRowThreads>(cnt, s_wave, &tot) - 1;  // run of position i0 - 1
#pragma unroll
    for (int j = 0; j < kRunPer; ++j) {
      const int64_t i = i0 + j;
      if (i >= n) break;
      const int64_t row = perm[i];
      if (head[j]) {
        ++run;
        if (run >= 0 && run < n) {
          offsets[run] = i;
          out.head(run, row, k[j]);
        }
      }
      if (row >= 0 && row < n) out.each(row, run);
    }
    __syncthreads();  // s_wave is rewritten by the next trip
  }
}

__device__ __forceinline__ int row_length(const int64_t* __restrict__ offsets, int64_t v) {
  const int64_t len = offsets[v + 1] - offsets[v];
  return (int)(len < INT_MAX ? len : INT_MAX);
}

// the longest row that any thread has seen: one integer atomic max per wave
__device__ __forceinline__ void longest_row_max(int longest, int32_t* __restrict__ dst) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) longest = max(longest, __shfl_xor(longest, d));
  if ((threadIdx.x & 63) == 0 && longest > 0) atomicMax(dst, longest);
}

// summary[1] = the longest of the summary[0] rows
template <int = 0>
__global__ __launch_bounds__(kRowThreads) void longest_row_kernel(const int64_t* __restrict__ offsets, int64_t n,
                                                                  int32_t* __restrict__ summary) {
  int64_t rows = summary[0];
  if (rows > n) rows = n;
  int longest = 0;
  for (int64_t v = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; v < rows; v += (int64_t)gridDim.x * kRowThreads)
    longest = max(longest, row_length(offsets, v));
  longest_row_max(longest, summary + 1);
}

// ---- c. long rows -----------------------------------------------------------------------------------------------------------
struct RowList {  // the long rows of a CSR and their chunks
  int32_t* counters;   // [0] chunk items, [1] long rows
  int32_t* item_row;   // [item_cap]
  int32_t* item_k;     // [item_cap] chunk number inside the row
  int32_t* long_row;   // [long_cap]
  int32_t* long_base;  // [long_cap] first item of the row
  int64_t item_cap, long_cap;
};

inline void row_list_caps(int64_t nnz, RowList& w) {
  w.long_cap = nnz / kRowChunk + 1;  // a long row holds more than kRowChunk entries
  w.item_cap = 2 * w.long_cap;       // ceil(len / chunk) <= len / chunk + 1 per long row
}

// one wave looks at 64 rows; every long one takes its run of items with one integer atomic and the wave writes the run
template <int = 0>
__global__ __launch_bounds__(kRowThreads) void row_list_collect_kernel(const int64_t* __restrict__ offsets, int64_t m,
                                                                       int64_t nnz, RowList w) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (kRowThreads / 64) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (kRowThreads / 64);
  for (int64_t base = wave * 64; base < m; base += nwaves * 64) {
    const int64_t row = base + lane;
    int nch = 0;
    if (row < m) {
      const int64_t j0 = offsets[row], j1 = offsets[row + 1];
      if (j0 >= 0 && j1 <= nnz && j1 - j0 > kRowChunk) nch = (int)((j1 - j0 + kRowChunk - 1) / kRowChunk);
    }
    unsigned long long todo = __ballot(nch > 0);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int s_row = (int)__shfl((int)row, src), s_n = __shfl(nch, src);
      int first = 0, slot = 0;
      if (lane == 0) {
        first = atomicAdd(w.counters, s_n);
        slot = atomicAdd(w.counters + 1, 1);
        if (slot < w.long_cap) {
          w.long_row[slot] = s_row;
          w.long_base[slot] = first;
        }
      }
      first = __shfl(first, 0);
      for (int k = lane; k < s_n; k += 64) {
        if ((int64_t)first + k < w.item_cap) {
          w.item_row[first + k] = s_row;
          w.item_k[first + k] = k;
        }
      }
    }
  }
}

__device__ __forceinline__ int64_t row_list_items(const RowList& w) {
  const int64_t total = w.counters[0];
  return total > w.item_cap ? w.item_cap : total;
}

__device__ __forceinline__ int64_t row_list_long_rows(const RowList& w) {
  const int64_t total = w.counters[1];
  return total > w.long_cap ? w.long_cap : total;
}

// entries [j0, j1) of `row`; offsets that do not describe the list: an empty row.  False: there is no such row.
__device__ __forceinline__ bool row_span(const int64_t* __restrict__ offsets, int64_t m, int64_t nnz, int64_t row, int64_t& j0,
                                         int64_t& j1) {
  if (row < 0 || row >= m) return false;
  j0 = offsets[row];
  j1 = offsets[row + 1];
  if (j0 < 0 || j1 > nnz || j1 < j0) j1 = j0 = 0;
  return true;
}

// item t of the list: its row and the entries [j0, j1) of its chunk
__device__ __forceinline__ bool row_list_item(const RowList& w, int64_t t, const int64_t* __restrict__ offsets, int64_t m,
                                              int64_t nnz, int64_t& row, int64_t& j0, int64_t& j1) {
  row = w.item_row[t];
  if (!row_span(offsets, m, nnz, row, j0, j1)) return false;
  j0 += (int64_t)w.item_k[t] * kRowChunk;
  if (j0 > j1) j0 = j1;
  if (j1 - j0 > kRowChunk) j1 = j0 + kRowChunk;
  return true;
}

// long row t of the list: its row, its length and its partials [first, first + nch).  False: the entry describes none.
__device__ __forceinline__ bool row_list_long_row(const RowList& w, int64_t t, const int64_t* __restrict__ offsets, int64_t m,
                                                  int64_t& row, int64_t& len, int64_t& first, int64_t& nch) {
  row = w.long_row[t];
  first = w.long_base[t];
  if (row < 0 || row >= m) return false;
  len = offsets[row + 1] - offsets[row];
  nch = (len + kRowChunk - 1) / kRowChunk;
  return first >= 0 && nch >= 1 && first + nch <= w.item_cap;
}

}  // namespace wcn
