// lattice.hip - high-dimensional filtering on sparse lattices: the permutohedral lattice and the bilateral grid (reference:
// nn/functional/permutohedral.py, bilateral_grid.py, bilateral.py and geometry/coords/search/packed128_hashmap.py, where a
// filter call is about 40 framework launches with float-atomic index_add_ and a neighbour search per call).
//
//   a. hash128       a table for keys of up to 7 axes of 17 bits.  A slot is claimed under linear probing by a 32-bit CAS on
//                    its VALUE word (-1 -> row); the two key words follow as one plain 16-B store.  Keys are distinct by
//                    contract, so an inserting thread never compares keys: a claimed slot is skipped.  Searches run in a later
//                    launch and read value first, key second.
//   b. geometry      one thread per point, everything in registers: the d + 1 simplex vertices and barycentric weights of the
//                    permutohedral lattice, or the 2^d corners and d-linear weights of the grid.  Every vertex key goes out as
//                    a (hi, lo) pair of 64-bit words, axis 0 in the most significant field, fields biased by 2^16, so that the
//                    unsigned order of the pair is the lexicographic order of the signed rows.  The top bit of `lo` is flipped:
//                    the framework's sort compares int64 as signed.
//   c. vertex map    sorted pairs + permutation -> unique keys (decoded), the vertex of every entry, CSR offsets by vertex and
//                    the longest row: the runs -> map kernels of row_lists.h on (hi, lo) pairs.
//   d. features      fp32 rows of `pitch` floats, pitch a multiple of 4: every row access is 16-B pieces.
//                    splat  out[v] = alpha * sum over e in row v of w[e] * f[e / K], ascending; rows longer than kRowChunk go
//                           by the chunk rule of row_lists.h, on a plan built once per CSR
//                    blur   y[v] = s0 x[v] + s1 x[n1[v]] + s2 x[n2[v]], -1 reads as zero
//                    slice  out[i] = alpha * sum over k of w[i, k] * x[idx[i, k]], -1 reads as zero
//   e. solver        the conjugate-gradient loop of the fast bilateral solver on the grid: 2 d + 2 launches an iteration, every
//                    scalar from per-workgroup fp64 partials added in index order, a state block instead of a host read
//   f. knn weights   the normalised weights of the kNN bilateral filter, one thread per query; the aggregation is the slice
// No float atomics anywhere: the bits of a result depend on the lattice alone.  The integer atomics (status word, longest row,
// the list of long rows) give the same result in any order.  Every grid is capped at kRowMaxGrid workgroups and strides.
#include "row_lists.h"

namespace wcn {

constexpr int kLtAxes = 7;                    // key fields
constexpr int kLtBits = 17;                   // bits of a field
constexpr int kLtSearchMax = 32;              // offsets of one batched search
constexpr int kLtCoordMin = -(1 << (kLtBits - 1));
constexpr int kLtCoordMax = (1 << (kLtBits - 1)) - 1;
constexpr uint64_t kLtField = (1ull << kLtBits) - 1;
constexpr uint64_t kLtSign = 1ull << 63;

struct Key128 {
  uint64_t hi, lo;
};

// append one field below the ones already there (the caller has checked the range)
__device__ __forceinline__ void key_push(Key128& k, int c) {
  k.hi = (k.hi << kLtBits) | (k.lo >> (64 - kLtBits));
  k.lo = (k.lo << kLtBits) | (uint64_t)(uint32_t)(c - kLtCoordMin);
}

__device__ __forceinline__ bool lt_in_range(int64_t c) { return c >= kLtCoordMin && c <= kLtCoordMax; }

// field j of a key of key_dim fields
__device__ __forceinline__ int key_field(const Key128& k, int key_dim, int j) {
  const int sh = kLtBits * (key_dim - 1 - j);
  uint64_t f;
  if (sh >= 64) f = k.hi >> (sh - 64);
  else if (sh == 0) f = k.lo;
  else f = (k.lo >> sh) | (k.hi << (64 - sh));
  return (int)(f & kLtField) + kLtCoordMin;
}

// ---- a. hash128 -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t h128_slot(const Key128& k, uint32_t mask) {
  return hash_slot(k.lo ^ (k.hi * 0x9E3779B97F4A7C15ull), mask);
}

__global__ __launch_bounds__(kRowThreads) void h128_insert_kernel(ulonglong2* __restrict__ tkeys, int32_t* __restrict__ tvals,
                                                                 uint32_t mask, const int32_t* __restrict__ coords, int64_t n,
                                                                 int key_dim, int32_t* __restrict__ status) {
  for (int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRowThreads) {
    Key128 k{0, 0};
    bool ok = true;
    for (int j = 0; j < key_dim; ++j) {
      const int c = coords[i * key_dim + j];
      ok = ok && lt_in_range(c);
      key_push(k, ok ? c : 0);
    }
    if (!ok) {
      atomicOr(status, WCN_FLAG_COORD_RANGE);
      continue;
    }
    uint32_t s = h128_slot(k, mask);
    bool placed = false;
    for (uint32_t attempts = 0; attempts <= mask; ++attempts) {
      if (atomicCAS(tvals + s, -1, (int32_t)i) == -1) {
        tkeys[s] = make_ulonglong2(k.hi, k.lo);
        placed = true;
        break;
      }
      s = (s + 1) & mask;
    }
    // n <= capacity distinct keys always find a slot, and the Python class refuses n > capacity before any launch (a thread of a
    // full table probes every slot): the flag is for direct callers of the C ABI
    if (!placed) atomicOr(status, WCN_FLAG_TABLE_FULL);
  }
}

__device__ __forceinline__ int h128_lookup(const ulonglong2* __restrict__ tkeys, const int32_t* __restrict__ tvals,
                                           uint32_t mask, const Key128& k) {
  uint32_t s = h128_slot(k, mask);
  for (uint32_t attempts = 0; attempts <= mask; ++attempts) {
    const int32_t v = tvals[s];
    if (v == -1) return -1;
    const ulonglong2 q = tkeys[s];
    if (q.x == k.hi && q.y == k.lo) return v;
    s = (s + 1) & mask;
  }
  return -1;
}

// out[k, i] = row of queries[i] + offsets[k], -1 when absent or outside the key range; offsets == null: one zero offset
__global__ __launch_bounds__(kRowThreads) void h128_search_kernel(const ulonglong2* __restrict__ tkeys,
                                                                 const int32_t* __restrict__ tvals, uint32_t mask,
                                                                 const int32_t* __restrict__ queries,
                                                                 const int32_t* __restrict__ offsets, int64_t m, int K,
                                                                 int key_dim, int32_t* __restrict__ out) {
  __shared__ int s_off[kLtSearchMax * kLtAxes];
  for (int t = threadIdx.x; t < K * key_dim; t += kRowThreads) s_off[t] = offsets ? offsets[t] : 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kRowThreads) {
    int c[kLtAxes];
#pragma unroll
    for (int j = 0; j < kLtAxes; ++j) c[j] = j < key_dim ? queries[i * key_dim + j] : 0;
    for (int k = 0; k < K; ++k) {
      Key128 key{0, 0};
      bool ok = true;
#pragma unroll
      for (int j = 0; j < kLtAxes; ++j) {
        if (j < key_dim) {
          const int64_t v = (int64_t)c[j] + s_off[k * key_dim + j];
          ok = ok && lt_in_range(v);
          key_push(key, ok ? (int)v : 0);
        }
      }
      out[(int64_t)k * m + i] = ok ? h128_lookup(tkeys, tvals, mask, key) : -1;
    }
  }
}

// ---- b. geometry ------------------------------------------------------------------------------------------------------------
struct LtScale {
  float v[kLtAxes - 1];
};

__device__ __forceinline__ void lt_emit(const Key128& k, bool ok, int64_t e, int64_t* __restrict__ key_hi,
                                        int64_t* __restrict__ key_lo) {
  if (key_hi) key_hi[e] = ok ? (int64_t)k.hi : 0;
  if (key_lo) key_lo[e] = ok ? (int64_t)(k.lo ^ kLtSign) : (int64_t)kLtSign;
}

// The arithmetic is the framework's, operation by operation and without contraction into FMAs (embed: product with the scale
// table, suffix sums; round to the nearest multiple of d + 1; rank the residuals, ties to the lower axis; correct the vertex to
// coordinate sum 0; weights as differences of neighbouring residuals), so an fp32 build on the host gives the same bits.
__global__ __launch_bounds__(kRowThreads) void permuto_simplex_kernel(const float* __restrict__ pos, int64_t n, int d, LtScale sc,
                                                                     int64_t* __restrict__ key_hi, int64_t* __restrict__ key_lo,
                                                                     int32_t* __restrict__ keys, float* __restrict__ bary,
                                                                     int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const int dp1 = d + 1;
  const float fdp1 = (float)dp1;
  const float inv = (float)(1.0 / (double)dp1);
  for (int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRowThreads) {
    float cf[kLtAxes - 1], el[kLtAxes];
#pragma unroll
    for (int j = 0; j < kLtAxes - 1; ++j) cf[j] = j < d ? pos[i * d + j] * sc.v[j] : 0.f;
    float sm = 0.f;
#pragma unroll
    for (int t = kLtAxes - 1; t >= 1; --t) {
      if (t <= d) {
        el[t] = sm - (float)t * cf[t - 1];
        sm = sm + cf[t - 1];
      } else {
        el[t] = 0.f;
      }
    }
    el[0] = sm;
    int g[kLtAxes], rank[kLtAxes];
    float diff[kLtAxes];
    bool ok = true;
    int sum = 0;
#pragma unroll
    for (int j = 0; j < kLtAxes; ++j) {
      g[j] = 0;
      diff[j] = 0.f;
      if (j < dp1) {
        const float v = el[j] * inv;
        const float up = ceilf(v) * fdp1, down = floorf(v) * fdp1;
        const float gr = (up - el[j]) < (el[j] - down) ? up : down;
        ok = ok && fabsf(gr) <= 1048576.f;  // NaN and anything the 17-bit fields cannot hold by far
        g[j] = ok ? (int)gr : 0;
        diff[j] = el[j] - gr;
        sum += g[j];
      }
    }
    if (!ok) {
      atomicOr(status, WCN_FLAG_COORD_RANGE);
      for (int k = 0; k < dp1; ++k) {
        lt_emit(Key128{0, 0}, false, i * dp1 + k, key_hi, key_lo);
        bary[i * dp1 + k] = 0.f;
        if (keys)
          for (int j = 0; j < dp1; ++j) keys[(i * dp1 + k) * dp1 + j] = 0;
      }
      continue;
    }
    const int sum_g = sum >= 0 ? sum / dp1 : -((-sum + dp1 - 1) / dp1);  // floor division
#pragma unroll
    for (int j = 0; j < kLtAxes; ++j) {
      int r = 0;
#pragma unroll
      for (int q = 0; q < kLtAxes; ++q)
        if (q < dp1 && j < dp1 && (diff[q] > diff[j] || (diff[q] == diff[j] && q < j))) ++r;
      rank[j] = r;
    }
    const int up_n = sum_g > 0 ? sum_g : 0, dn_n = sum_g < 0 ? -sum_g : 0;
    float delta[kLtAxes];
#pragma unroll
    for (int j = 0; j < kLtAxes; ++j) {
      delta[j] = 0.f;
      if (j < dp1) {
        const int shift = ((rank[j] < dn_n) ? dp1 : 0) - ((rank[j] >= dp1 - up_n) ? dp1 : 0);
        g[j] += shift;
        rank[j] += sum_g + shift;
        delta[j] = (el[j] - (float)g[j]) * inv;
      }
    }
    // weight t = residual of the axis with rank d - t, minus the residual of the axis with rank d + 1 - t
    float b[kLtAxes];
    float wrap = 0.f;
#pragma unroll
    for (int t = 0; t < kLtAxes; ++t) {
      float plus = 0.f, minus = 0.f;
#pragma unroll
      for (int j = 0; j < kLtAxes; ++j) {
        if (j < dp1) {
          plus = rank[j] == d - t ? delta[j] : plus;
          minus = rank[j] == d + 1 - t ? delta[j] : minus;
        }
      }
      b[t] = plus - minus;
    }
#pragma unroll
    for (int j = 0; j < kLtAxes; ++j)
      if (j < dp1 && rank[j] == 0) wrap = -delta[j];
    b[0] = (b[0] + 1.0f) + wrap;
    bool all_ok = true;
#pragma unroll
    for (int k = 0; k < kLtAxes; ++k) {
      if (k < dp1) {
        Key128 key{0, 0};
        bool kok = true;
        const int64_t e = i * dp1 + k;
#pragma unroll
        for (int j = 0; j < kLtAxes; ++j) {
          if (j < dp1) {
            const int c = g[j] + (rank[j] <= d - k ? k : k - dp1);
            kok = kok && lt_in_range(c);
            key_push(key, kok ? c : 0);
            if (keys) keys[e * dp1 + j] = c;
          }
        }
        lt_emit(key, kok, e, key_hi, key_lo);
        bary[e] = b[k];
        all_ok = all_ok && kok;
      }
    }
    if (!all_ok) atomicOr(status, WCN_FLAG_COORD_RANGE);
  }
}

// corner c of a point: bit (d - 1 - j) of c steps axis j, the order of itertools.product([0, 1], repeat=d)
__global__ __launch_bounds__(kRowThreads) void grid_corners_kernel(const float* __restrict__ pos, int64_t n, int d,
                                                                  int64_t* __restrict__ floors, int64_t* __restrict__ key_hi,
                                                                  int64_t* __restrict__ key_lo, int32_t* __restrict__ keys,
                                                                  float* __restrict__ weights, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const int K = 1 << d;
  for (int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRowThreads) {
    int fl[kLtAxes - 1];
    float fr[kLtAxes - 1];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < kLtAxes - 1; ++j) {
      fl[j] = 0;
      fr[j] = 0.f;
      if (j < d) {
        const float p = pos[i * d + j], f = floorf(p);
        ok = ok && f >= (float)kLtCoordMin && f <= (float)kLtCoordMax;  // the floor itself; its upper corner is judged per corner
        fl[j] = ok ? (int)f : 0;
        fr[j] = p - f;
        if (floors) floors[i * d + j] = fl[j];
      }
    }
    bool all_ok = ok;
    for (int c = 0; c < K; ++c) {
      Key128 key{0, 0};
      bool kok = ok;
      float w = 1.f;
      const int64_t e = i * K + c;
#pragma unroll
      for (int j = 0; j < kLtAxes - 1; ++j) {
        if (j < d) {
          const int bit = (c >> (d - 1 - j)) & 1;
          w = w * (bit ? fr[j] : 1.f - fr[j]);
          kok = kok && lt_in_range(fl[j] + bit);
          key_push(key, kok ? fl[j] + bit : 0);
          if (keys) keys[e * d + j] = fl[j] + bit;  // a corner one past the range: the search reports it absent
        }
      }
      lt_emit(key, kok, e, key_hi, key_lo);
      weights[e] = ok ? w : 0.f;  // a point whose floor is outside the range (NaN included) weighs nothing
      all_ok = all_ok && kok;
    }
    if (!all_ok) atomicOr(status, WCN_FLAG_COORD_RANGE);
  }
}

// ---- c. runs -> vertex map --------------------------------------------------------------------------------------------------
struct LtKeys {  // key policy of row_lists.h: a (hi, lo) pair per position, hi absent where the fields fit one word
  struct Key {
    int64_t hi, lo;
  };
  const int64_t* hi;
  const int64_t* lo;
  __device__ __forceinline__ void load(int64_t n, int64_t i0, Key (&k)[kRunPer]) const {
#pragma unroll
    for (int j = 0; j < kRunPer; ++j) {
      k[j].hi = (hi && i0 + j < n) ? hi[i0 + j] : 0;
      k[j].lo = i0 + j < n ? lo[i0 + j] : 0;
    }
  }
  __device__ __forceinline__ Key at(int64_t i) const { return Key{hi ? hi[i] : 0, lo[i]}; }
  static __device__ __forceinline__ bool differ(const Key& a, const Key& b) { return a.hi != b.hi || a.lo != b.lo; }
};

struct LtWriter {  // what a vertex and an entry get
  int key_dim;
  int32_t* unique_keys;
  int64_t* inverse;
  __device__ __forceinline__ void head(int64_t vid, int64_t, const LtKeys::Key& key) const {
    const Key128 k{(uint64_t)key.hi, (uint64_t)key.lo ^ kLtSign};
    for (int a = 0; a < key_dim; ++a) unique_keys[vid * key_dim + a] = key_field(k, key_dim, a);
  }
  __device__ __forceinline__ void each(int64_t e, int64_t vid) const { inverse[e] = vid; }
};

// ---- long rows: the chunk plan of a CSR -------------------------------------------------------------------------------------
// the list in the int32 words of the caller's plan buffer, packed; *ints = the words it takes
static RowList lt_carve(int32_t* base, int64_t nnz, int64_t* ints = nullptr) {
  RowList p;
  row_list_caps(nnz, p);
  int64_t at = 0;
  p.counters = base + at;
  at += kRowListCounterInts;
  p.item_row = base + at;
  at += p.item_cap;
  p.item_k = base + at;
  at += p.item_cap;
  p.long_row = base + at;
  at += p.long_cap;
  p.long_base = base + at;
  at += p.long_cap;
  if (ints) *ints = at;
  return p;
}

// ---- d. feature kernels -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 f4_fma(float a, const float4& x, const float4& acc) {
  return make_float4(fmaf(a, x.x, acc.x), fmaf(a, x.y, acc.y), fmaf(a, x.z, acc.z), fmaf(a, x.w, acc.w));
}
__device__ __forceinline__ float4 f4_scale(float a, const float4& x) { return make_float4(a * x.x, a * x.y, a * x.z, a * x.w); }

// entries [j0, j1) of one row, ascending, four loads in flight: acc += w[e] * f[e / K]
__device__ __forceinline__ float4 lt_row_sum(const float4* __restrict__ f, const float* __restrict__ w,
                                             const int64_t* __restrict__ entries, int64_t j0, int64_t j1, int64_t nnz,
                                             uint32_t K, int P4, int p) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int64_t j = j0;
  for (; j + 4 <= j1; j += 4) {
    float wt[4];
    float4 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t e = entries[j + u];
      const bool ok = e >= 0 && e < nnz;
      wt[u] = ok ? w[e] : 0.f;
      x[u] = ok ? f[(int64_t)((uint32_t)e / K) * P4 + p] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = f4_fma(wt[u], x[u], acc);
  }
  for (; j < j1; ++j) {
    const int64_t e = entries[j];
    if (e >= 0 && e < nnz) acc = f4_fma(w[e], f[(int64_t)((uint32_t)e / K) * P4 + p], acc);
  }
  return acc;
}

// L lanes (a power of two <= 64) own one list: ITEMS = false, a whole row (longer ones are skipped when `split`); ITEMS = true,
// one chunk of a long row into the partials.  Rows wider than L pieces take several trips.
template <bool ITEMS>
__global__ __launch_bounds__(kRowThreads) void lt_splat_kernel(const float4* __restrict__ f, const float* __restrict__ w,
                                                              const int64_t* __restrict__ offsets,
                                                              const int64_t* __restrict__ entries, int64_t m, int64_t nnz,
                                                              uint32_t K, int P4, int L, float alpha, int split,
                                                              float4* __restrict__ out, RowList plan, float4* __restrict__ part) {
  const int groups = kRowThreads / L;
  const int g = threadIdx.x / L, sub = threadIdx.x % L;
  const int64_t total = ITEMS ? row_list_items(plan) : m;
  for (int64_t t = (int64_t)blockIdx.x * groups + g; t < total; t += (int64_t)gridDim.x * groups) {
    int64_t row = t, j0, j1;
    if (!(ITEMS ? row_list_item(plan, t, offsets, m, nnz, row, j0, j1) : row_span(offsets, m, nnz, row, j0, j1))) continue;
    if (!ITEMS && split && j1 - j0 > kRowChunk) continue;
    for (int p = sub; p < P4; p += L) {
      const float4 acc = lt_row_sum(f, w, entries, j0, j1, nnz, K, P4, p);
      if (ITEMS) part[t * P4 + p] = acc;
      else out[row * P4 + p] = f4_scale(alpha, acc);
    }
  }
}

// L lanes per long row: its partials in chunk order
__global__ __launch_bounds__(kRowThreads) void lt_combine_kernel(const int64_t* __restrict__ offsets, int64_t m, int P4, int L,
                                                                float alpha, float4* __restrict__ out, RowList plan,
                                                                const float4* __restrict__ part) {
  const int groups = kRowThreads / L;
  const int g = threadIdx.x / L, sub = threadIdx.x % L;
  const int64_t total = row_list_long_rows(plan);
  for (int64_t t = (int64_t)blockIdx.x * groups + g; t < total; t += (int64_t)gridDim.x * groups) {
    int64_t row, len, first, nch;
    if (!row_list_long_row(plan, t, offsets, m, row, len, first, nch)) continue;
    for (int p = sub; p < P4; p += L) {
      float4 acc = part[first * P4 + p];
      for (int64_t k = 1; k < nch; ++k) {
        const float4 q = part[(first + k) * P4 + p];
        acc = make_float4(acc.x + q.x, acc.y + q.y, acc.z + q.z, acc.w + q.w);
      }
      out[row * P4 + p] = f4_scale(alpha, acc);
    }
  }
}

__device__ __forceinline__ float4 lt_row_or_zero(const float4* __restrict__ x, int64_t r, int64_t m, int P4, int p) {
  return (r >= 0 && r < m) ? x[r * P4 + p] : make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(kRowThreads) void lt_blur_kernel(const float4* __restrict__ x, const int32_t* __restrict__ n1,
                                                             const int32_t* __restrict__ n2, float s0, float s1, float s2,
                                                             int64_t m, int P4, int L, float4* __restrict__ y) {
  const int groups = kRowThreads / L;
  const int g = threadIdx.x / L, sub = threadIdx.x % L;
  for (int64_t v = (int64_t)blockIdx.x * groups + g; v < m; v += (int64_t)gridDim.x * groups) {
    const int64_t a = n1[v], b = n2 ? n2[v] : -1;
    for (int p = sub; p < P4; p += L) {
      const float4 xa = lt_row_or_zero(x, a, m, P4, p), xb = lt_row_or_zero(x, b, m, P4, p);
      float4 acc = f4_scale(s0, x[v * P4 + p]);
      acc = f4_fma(s1, xa, acc);
      if (n2) acc = f4_fma(s2, xb, acc);
      y[v * P4 + p] = acc;
    }
  }
}

__global__ __launch_bounds__(kRowThreads) void lt_slice_kernel(const float4* __restrict__ x, const int64_t* __restrict__ idx,
                                                              const float* __restrict__ w, int64_t n, int K, int64_t m, int P4,
                                                              int L, float alpha, float4* __restrict__ out) {
  const int groups = kRowThreads / L;
  const int g = threadIdx.x / L, sub = threadIdx.x % L;
  for (int64_t i = (int64_t)blockIdx.x * groups + g; i < n; i += (int64_t)gridDim.x * groups) {
    for (int p = sub; p < P4; p += L) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = 0; k < K; ++k) {
        const int64_t r = idx[i * K + k];
        if (r >= 0 && r < m) acc = f4_fma(w[i * K + k], x[r * P4 + p], acc);
      }
      out[i * P4 + p] = f4_scale(alpha, acc);
    }
  }
}

// ---- e. the bilateral solver's conjugate-gradient loop (reference: bilateral_solver of nn/functional/bilateral_grid.py) -------
// A p = (lam D + C) p - lam n blur(n p) over fp32 rows; 2 d blur passes of which the first folds the n p scaling into its gather
// and the last forms A p and one partial of sum p . A p per workgroup.  Every scalar of the loop is the sum of per-workgroup
// partials: products and sums in fp64, xor butterflies inside a wave, the waves in order, the partials in index order by every
// workgroup that needs the scalar.  The state block (doubles) carries rz_old and the done flag twice, by iteration parity: the
// direction kernel of iteration `it` reads slot it & 1 and its workgroup 0 writes slot (it + 1) & 1, which only later launches
// read, so no launch reads a word that the same launch writes.
constexpr int kPcgRz = 0;         // [2] sum r . z the iteration starts from
constexpr int kPcgNorm0 = 2;      // max(|r0|, 1e-20)
constexpr int kPcgDone = 3;       // [2] non-zero: the stop test has held, every launch returns without writing
constexpr int kPcgIters = 5;      // updates of y carried out
constexpr int kPcgNonFinite = 6;  // a residual norm was not finite
constexpr int kPcgWords = 8;

// the workgroup's sum of one double per thread, the same bits in every thread; `s_red`: kRowThreads / 64 doubles
__device__ __forceinline__ double lt_block_sum(double v, double* s_red) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();  // s_red may still be read by the call before
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < kRowThreads / 64; ++w) t += s_red[w];
  return t;
}

__device__ __forceinline__ double lt_sum_partials(const double* __restrict__ part, int n, double* s_red) {
  double acc = 0.0;
  for (int j = threadIdx.x; j < n; j += kRowThreads) acc += part[j];
  return lt_block_sum(acc, s_red);
}

__device__ __forceinline__ double f4_dot(const float4& a, const float4& b) {
  return (double)a.x * (double)b.x + (double)a.y * (double)b.y + (double)a.z * (double)b.z + (double)a.w * (double)b.w;
}

__device__ __forceinline__ double clamp_min_keep_nan(double v, double lo) { return v < lo ? lo : v; }

// the first pass of the matvec: a blur pass over scale[.] * x[.]
__global__ __launch_bounds__(kRowThreads) void lt_blur_scaled_kernel(const float4* __restrict__ x, const float* __restrict__ scale,
                                                                    const int32_t* __restrict__ n1, float s0, float s1, int64_t m,
                                                                    int P4, int L, const double* __restrict__ skip,
                                                                    float4* __restrict__ y) {
  if (skip && *skip != 0.0) return;
  const int groups = kRowThreads / L;
  const int g = threadIdx.x / L, sub = threadIdx.x % L;
  for (int64_t v = (int64_t)blockIdx.x * groups + g; v < m; v += (int64_t)gridDim.x * groups) {
    const int64_t a = n1[v];
    const float sv = scale[v], sa = (a >= 0 && a < m) ? scale[a] : 0.f;
    for (int p = sub; p < P4; p += L) {
      const float4 xa = f4_scale(sa, lt_row_or_zero(x, a, m, P4, p));
      y[v * P4 + p] = f4_fma(s1, xa, f4_scale(s0, f4_scale(sv, x[v * P4 + p])));
    }
  }
}

// the last pass: t = s0 x[v] + s1 x[n1[v]], Ap[v] = dc[v] p[v] - lam n[v] t, partial[workgroup] = sum p . Ap
__global__ __launch_bounds__(kRowThreads) void lt_matvec_last_kernel(const float4* __restrict__ x, const int32_t* __restrict__ n1,
                                                                    float s0, float s1, const float4* __restrict__ pv,
                                                                    const float* __restrict__ nvec, const float* __restrict__ dc,
                                                                    float lam, int64_t m, int P4, int L,
                                                                    const double* __restrict__ skip, float4* __restrict__ Ap,
                                                                    double* __restrict__ partial) {
  __shared__ double s_red[kRowThreads / 64];
  if (skip && *skip != 0.0) return;
  const int groups = kRowThreads / L;
  const int g = threadIdx.x / L, sub = threadIdx.x % L;
  double sum = 0.0;
  for (int64_t v = (int64_t)blockIdx.x * groups + g; v < m; v += (int64_t)gridDim.x * groups) {
    const int64_t a = n1[v];
    const float dv = dc[v], ln = lam * nvec[v];
    for (int p = sub; p < P4; p += L) {
      const float4 t = f4_fma(s1, lt_row_or_zero(x, a, m, P4, p), f4_scale(s0, x[v * P4 + p]));
      const float4 q = pv[v * P4 + p];
      const float4 ap = make_float4(fmaf(dv, q.x, -(ln * t.x)), fmaf(dv, q.y, -(ln * t.y)), fmaf(dv, q.z, -(ln * t.z)),
                                    fmaf(dv, q.w, -(ln * t.w)));
      Ap[v * P4 + p] = ap;
      sum += f4_dot(q, ap);
    }
  }
  sum = lt_block_sum(sum, s_red);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// INIT: r = tbar - Ap (Ap = A y0), z = minv r, p = z.  Otherwise alpha = rz_old / max(sum of the p . Ap partials, 1e-20),
// y += alpha p, r -= alpha Ap, z = minv r.  Both leave the partials of sum r . r and sum r . z.
template <bool INIT>
__global__ __launch_bounds__(kRowThreads) void lt_pcg_update_kernel(const double* __restrict__ st, int it,
                                                                   const double* __restrict__ pap_part, int nparts,
                                                                   float4* __restrict__ p, const float4* __restrict__ Ap,
                                                                   const float* __restrict__ minv, const float4* __restrict__ tbar,
                                                                   float4* __restrict__ y, float4* __restrict__ r,
                                                                   float4* __restrict__ z, int64_t m, int P4, int L,
                                                                   double* __restrict__ rr_part, double* __restrict__ rz_part) {
  __shared__ double s_red[kRowThreads / 64];
  float alpha = 0.f;
  if (!INIT) {
    if (st[kPcgDone + (it & 1)] != 0.0) return;
    const double pap = lt_sum_partials(pap_part, nparts, s_red);
    alpha = (float)(st[kPcgRz + (it & 1)] / clamp_min_keep_nan(pap, 1e-20));
  }
  const int groups = kRowThreads / L;
  const int g = threadIdx.x / L, sub = threadIdx.x % L;
  double rr = 0.0, rz = 0.0;
  for (int64_t v = (int64_t)blockIdx.x * groups + g; v < m; v += (int64_t)gridDim.x * groups) {
    const float mi = minv[v];
    for (int q = sub; q < P4; q += L) {
      const int64_t at = v * P4 + q;
      const float4 ap = Ap[at];
      float4 rv;
      if (INIT) {
        const float4 t = tbar[at];
        rv = make_float4(t.x - ap.x, t.y - ap.y, t.z - ap.z, t.w - ap.w);
      } else {
        y[at] = f4_fma(alpha, p[at], y[at]);
        rv = f4_fma(-alpha, ap, r[at]);
      }
      const float4 zv = f4_scale(mi, rv);
      r[at] = rv;
      z[at] = zv;
      if (INIT) p[at] = zv;
      rr += f4_dot(rv, rv);
      rz += f4_dot(rv, zv);
    }
  }
  rr = lt_block_sum(rr, s_red);
  rz = lt_block_sum(rz, s_red);
  if (threadIdx.x == 0) {
    rr_part[blockIdx.x] = rr;
    rz_part[blockIdx.x] = rz;
  }
}

// ONE workgroup: the state block from the partials of the first residual
__global__ __launch_bounds__(kRowThreads) void lt_pcg_start_kernel(double* __restrict__ st, const double* __restrict__ rr_part,
                                                                  const double* __restrict__ rz_part, int nparts) {
  __shared__ double s_red[kRowThreads / 64];
  const double rr = lt_sum_partials(rr_part, nparts, s_red), rz = lt_sum_partials(rz_part, nparts, s_red);
  if (threadIdx.x == 0) {
    const double norm = sqrt(rr);
    st[kPcgRz] = rz;
    st[kPcgRz + 1] = 0.0;
    st[kPcgNorm0] = clamp_min_keep_nan(norm, 1e-20);
    st[kPcgDone] = st[kPcgDone + 1] = 0.0;
    st[kPcgIters] = 0.0;
    st[kPcgNonFinite] = isfinite(norm) ? 0.0 : 1.0;
    st[kPcgWords - 1] = 0.0;
  }
}

// the stop test |r| / |r0| < tol on the reduced norm, then beta = rz_new / max(rz_old, 1e-20), p = z + beta p
__global__ __launch_bounds__(kRowThreads) void lt_pcg_direction_kernel(double* __restrict__ st, int it, double tol,
                                                                      const double* __restrict__ rr_part,
                                                                      const double* __restrict__ rz_part, int nparts,
                                                                      const float4* __restrict__ z, float4* __restrict__ p,
                                                                      int64_t m, int P4, int L) {
  __shared__ double s_red[kRowThreads / 64];
  const int cur = it & 1, nxt = cur ^ 1;
  if (st[kPcgDone + cur] != 0.0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) st[kPcgDone + nxt] = 1.0;
    return;
  }
  const double rr = lt_sum_partials(rr_part, nparts, s_red), rz_new = lt_sum_partials(rz_part, nparts, s_red);
  const double norm = sqrt(rr);
  const bool stop = norm / st[kPcgNorm0] < tol;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st[kPcgIters] = (double)(it + 1);
    st[kPcgDone + nxt] = stop ? 1.0 : 0.0;
    st[kPcgRz + nxt] = rz_new;
    if (!isfinite(norm)) st[kPcgNonFinite] = 1.0;
  }
  if (stop) return;
  const float beta = (float)(rz_new / clamp_min_keep_nan(st[kPcgRz + cur], 1e-20));
  const int groups = kRowThreads / L;
  const int g = threadIdx.x / L, sub = threadIdx.x % L;
  for (int64_t v = (int64_t)blockIdx.x * groups + g; v < m; v += (int64_t)gridDim.x * groups)
    for (int q = sub; q < P4; q += L) p[v * P4 + q] = f4_fma(beta, p[v * P4 + q], z[v * P4 + q]);
}

// ---- f. weights of the kNN bilateral filter (reference: nn/functional/bilateral.py) ---------------------------------------------
// one thread per query: w[s] = exp(-|dxyz|^2 ix - |dfeat|^2 if) over its k neighbours, the row sum in slot order, then
// w / max(sum, 1e-20).  A neighbour index outside [0, n) weighs nothing.
__global__ __launch_bounds__(kRowThreads) void bilateral_knn_weights_kernel(const float* __restrict__ src_xyz,
                                                                           const float* __restrict__ src_feat,
                                                                           const float* __restrict__ q_xyz,
                                                                           const float* __restrict__ q_feat,
                                                                           const int64_t* __restrict__ nbr, int64_t n, int64_t m,
                                                                           int K, int dx, int df, float inv_xyz, float inv_feat,
                                                                           float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kRowThreads) {
    float sum = 0.f;
    for (int s = 0; s < K; ++s) {
      const int64_t r = nbr[i * K + s];
      float w = 0.f;
      if (r >= 0 && r < n) {
        float a = 0.f, b = 0.f;
        for (int j = 0; j < dx; ++j) {
          const float t = src_xyz[r * dx + j] - q_xyz[i * dx + j];
          a = fmaf(t, t, a);
        }
        for (int j = 0; j < df; ++j) {
          const float t = src_feat[r * df + j] - q_feat[i * df + j];
          b = fmaf(t, t, b);
        }
        w = expf(-a * inv_xyz - b * inv_feat);
      }
      out[i * K + s] = w;
      sum += w;
    }
    const float den = sum < 1e-20f ? 1e-20f : sum;
    for (int s = 0; s < K; ++s) out[i * K + s] = out[i * K + s] / den;
  }
}

static bool lt_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace wcn

using namespace wcn;

extern "C" {

int32_t wcn_lattice_chunk_rows(void) { return kRowChunk; }

int wcn_hash128_insert(int64_t* table_keys, int32_t* table_values, int64_t capacity, const int32_t* coords, int64_t n,
                       int32_t key_dim, int32_t* status, wcn_stream_t stream) {
  if (!lt_pow2(capacity) || capacity > (1ll << 31) || n < 0 || n > INT32_MAX || key_dim < 1 || key_dim > kLtAxes ||
      !table_keys || !table_values || !status || !aligned_to(table_keys, 16) || (n > 0 && !coords))
    return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(table_values, 0xFF, (size_t)capacity * 4, s) != hipSuccess) return WCN_ERROR_KERNEL_EXECUTION;
  if (n == 0) return WCN_SUCCESS;
  hipLaunchKernelGGL(h128_insert_kernel, dim3(capped_grid(ceil_div(n, kRowThreads))), dim3(kRowThreads), 0, s,
                     (ulonglong2*)table_keys, table_values, (uint32_t)(capacity - 1), coords, n, (int)key_dim, status);
  return launch_status();
}

int wcn_hash128_search(const int64_t* table_keys, const int32_t* table_values, int64_t capacity, const int32_t* queries,
                       const int32_t* offsets, int64_t m, int32_t k, int32_t key_dim, int32_t* out, wcn_stream_t stream) {
  if (!lt_pow2(capacity) || capacity > (1ll << 31) || m < 0 || m > INT32_MAX || k < 1 || k > kLtSearchMax || key_dim < 1 ||
      key_dim > kLtAxes || !table_keys || !table_values || !aligned_to(table_keys, 16))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (m == 0) return WCN_SUCCESS;
  if (!queries || !out) return WCN_ERROR_INVALID_PARAMETERS;
  hipLaunchKernelGGL(h128_search_kernel, dim3(capped_grid(ceil_div(m, kRowThreads))), dim3(kRowThreads), 0, (hipStream_t)stream,
                     (const ulonglong2*)table_keys, table_values, (uint32_t)(capacity - 1), queries, offsets, m, (int)k,
                     (int)key_dim, out);
  return launch_status();
}

static int geometry_args_ok(const float* positions, int64_t n, int32_t d, int64_t entries_per_point, const float* weights,
                            const int32_t* status) {
  if (n < 0 || d < 1 || d > kLtAxes - 1 || !status || n * entries_per_point > INT32_MAX) return WCN_ERROR_INVALID_PARAMETERS;
  if (n > 0 && (!positions || !weights)) return WCN_ERROR_INVALID_PARAMETERS;
  return WCN_SUCCESS;
}

int wcn_permuto_simplex(const float* positions, int64_t n, int32_t d, const float* scale, int64_t* key_hi, int64_t* key_lo,
                        int32_t* keys, float* bary, int32_t* status, wcn_stream_t stream) {
  const int st = geometry_args_ok(positions, n, d, (int64_t)d + 1, bary, status);
  if (st != WCN_SUCCESS) return st;
  if (!scale) return WCN_ERROR_INVALID_PARAMETERS;
  if (n == 0) return WCN_SUCCESS;
  LtScale sc{};
  for (int j = 0; j < d; ++j) sc.v[j] = scale[j];
  hipLaunchKernelGGL(permuto_simplex_kernel, dim3(capped_grid(ceil_div(n, kRowThreads))), dim3(kRowThreads), 0, (hipStream_t)stream,
                     positions, n, (int)d, sc, key_hi, key_lo, keys, bary, status);
  return launch_status();
}

int wcn_grid_corners(const float* positions, int64_t n, int32_t d, int64_t* floors, int64_t* key_hi, int64_t* key_lo,
                     int32_t* keys, float* weights, int32_t* status, wcn_stream_t stream) {
  const int st = geometry_args_ok(positions, n, d, d >= 1 && d < kLtAxes ? (int64_t)1 << d : 1, weights, status);
  if (st != WCN_SUCCESS) return st;
  if (n == 0) return WCN_SUCCESS;
  hipLaunchKernelGGL(grid_corners_kernel, dim3(capped_grid(ceil_div(n, kRowThreads))), dim3(kRowThreads), 0, (hipStream_t)stream,
                     positions, n, (int)d, floors, key_hi, key_lo, keys, weights, status);
  return launch_status();
}

size_t wcn_lattice_map_workspace_bytes(int64_t nnz) {
  if (nnz < 0) return 0;
  return align256((size_t)ceil_div(nnz > 0 ? nnz : 1, kRunTile) * 4);
}

int wcn_lattice_map(const int64_t* sorted_hi, const int64_t* sorted_lo, const int64_t* perm, int64_t nnz, int32_t key_dim,
                    int32_t* unique_keys, int64_t* inverse, int64_t* row_offsets, int32_t* summary, void* workspace,
                    size_t workspace_bytes, wcn_stream_t stream) {
  if (nnz < 0 || nnz > INT32_MAX || key_dim < 1 || key_dim > kLtAxes || !summary || !row_offsets)
    return WCN_ERROR_INVALID_PARAMETERS;
  if (nnz > 0 && (!sorted_lo || !perm || !unique_keys || !inverse || !workspace ||
                  workspace_bytes < wcn_lattice_map_workspace_bytes(nnz) || (!sorted_hi && key_dim * kLtBits > 64)))
    return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(summary, 0, 8, s) != hipSuccess || hipMemsetAsync(row_offsets, 0, 8, s) != hipSuccess)
    return WCN_ERROR_KERNEL_EXECUTION;
  if (nnz == 0) return WCN_SUCCESS;
  const int64_t ntiles = ceil_div(nnz, kRunTile);
  int32_t* tile_sum = (int32_t*)workspace;
  const dim3 block(kRowThreads), tiles(capped_grid(ntiles));
  const LtKeys keys{sorted_hi, sorted_lo};
  hipLaunchKernelGGL(run_count_kernel<LtKeys>, tiles, block, 0, s, keys, nnz, ntiles, tile_sum);
  hipLaunchKernelGGL(run_scan_kernel<>, dim3(1), block, 0, s, tile_sum, ntiles, nnz, summary, row_offsets);
  hipLaunchKernelGGL((run_apply_kernel<LtKeys, LtWriter>), tiles, block, 0, s, keys, perm, nnz, ntiles, (const int32_t*)tile_sum,
                     row_offsets, LtWriter{(int)key_dim, unique_keys, inverse});
  hipLaunchKernelGGL(longest_row_kernel<>, dim3(capped_grid(ceil_div(nnz, kRowThreads))), block, 0, s, row_offsets, nnz,
                     summary);
  return launch_status();
}

int64_t wcn_lattice_plan_items(int64_t nnz) { return nnz < 0 ? 0 : lt_carve(nullptr, nnz).item_cap; }
int64_t wcn_lattice_plan_ints(int64_t nnz) {
  int64_t ints = 0;
  if (nnz >= 0) lt_carve(nullptr, nnz, &ints);
  return ints;
}

int wcn_lattice_plan(const int64_t* row_offsets, int64_t v, int64_t nnz, int32_t* plan, wcn_stream_t stream) {
  if (v < 0 || v > INT32_MAX || nnz < 0 || nnz > INT32_MAX || !plan || (v > 0 && !row_offsets))
    return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(plan, 0, kRowListCounterInts * 4, s) != hipSuccess) return WCN_ERROR_KERNEL_EXECUTION;
  if (v == 0) return WCN_SUCCESS;
  hipLaunchKernelGGL(row_list_collect_kernel<>, dim3(capped_grid(ceil_div(v, kRowThreads))), dim3(kRowThreads), 0, s,
                     row_offsets, v, nnz, lt_carve(plan, nnz));
  return launch_status();
}

static bool feature_args_ok(int64_t rows, int32_t pitch, const void* a, const void* b) {
  return rows >= 0 && rows <= INT32_MAX && pitch >= 4 && pitch % 4 == 0 && aligned_to(a, 16) && aligned_to(b, 16);
}

int wcn_lattice_splat(const float* f, const float* w, const int64_t* row_offsets, const int64_t* row_entries, int64_t v,
                      int64_t nnz, int32_t k, int32_t pitch, float alpha, const int32_t* plan, float* partials, float* out,
                      wcn_stream_t stream) {
  if (!feature_args_ok(v, pitch, f, out) || nnz < 0 || nnz > INT32_MAX || k < 1 || !aligned_to(partials, 16) ||
      (plan && !partials))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (v == 0) return WCN_SUCCESS;
  if (!out || !row_offsets || (nnz > 0 && (!f || !w || !row_entries))) return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  const int P4 = pitch / 4, L = row_lanes(P4), groups = kRowThreads / L;
  const RowList p = plan ? lt_carve(const_cast<int32_t*>(plan), nnz) : RowList{};
  hipLaunchKernelGGL(lt_splat_kernel<false>, dim3(capped_grid(ceil_div(v, groups))), dim3(kRowThreads), 0, s, (const float4*)f, w,
                     row_offsets, row_entries, v, nnz, (uint32_t)k, P4, L, alpha, plan ? 1 : 0, (float4*)out, p,
                     (float4*)partials);
  if (!plan) return launch_status();
  hipLaunchKernelGGL(lt_splat_kernel<true>, dim3(capped_grid(ceil_div(p.item_cap, groups))), dim3(kRowThreads), 0, s,
                     (const float4*)f, w, row_offsets, row_entries, v, nnz, (uint32_t)k, P4, L, alpha, 1, (float4*)out, p,
                     (float4*)partials);
  hipLaunchKernelGGL(lt_combine_kernel, dim3(capped_grid(ceil_div(p.long_cap, groups))), dim3(kRowThreads), 0, s, row_offsets, v, P4,
                     L, alpha, (float4*)out, p, (const float4*)partials);
  return launch_status();
}

int wcn_lattice_blur(const float* x, const int32_t* n1, const int32_t* n2, float s0, float s1, float s2, int64_t v,
                     int32_t pitch, float* y, wcn_stream_t stream) {
  if (!feature_args_ok(v, pitch, x, y) || x == y) return WCN_ERROR_INVALID_PARAMETERS;
  if (v == 0) return WCN_SUCCESS;
  if (!x || !y || !n1) return WCN_ERROR_INVALID_PARAMETERS;
  const int P4 = pitch / 4, L = row_lanes(P4);
  hipLaunchKernelGGL(lt_blur_kernel, dim3(capped_grid(ceil_div(v, kRowThreads / L))), dim3(kRowThreads), 0, (hipStream_t)stream,
                     (const float4*)x, n1, n2, s0, s1, s2, v, P4, L, (float4*)y);
  return launch_status();
}

int wcn_lattice_slice(const float* x, const int64_t* idx, const float* w, int64_t n, int32_t k, int64_t v, int32_t pitch,
                      float alpha, float* out, wcn_stream_t stream) {
  if (!feature_args_ok(n, pitch, x, out) || v < 0 || v > INT32_MAX || k < 1 || n * (int64_t)k > INT32_MAX)
    return WCN_ERROR_INVALID_PARAMETERS;
  if (n == 0) return WCN_SUCCESS;
  if (!out || !idx || !w || (v > 0 && !x)) return WCN_ERROR_INVALID_PARAMETERS;
  const int P4 = pitch / 4, L = row_lanes(P4);
  hipLaunchKernelGGL(lt_slice_kernel, dim3(capped_grid(ceil_div(n, kRowThreads / L))), dim3(kRowThreads), 0, (hipStream_t)stream,
                     (const float4*)x, idx, w, n, (int)k, v, P4, L, alpha, (float4*)out);
  return launch_status();
}

// ---- the bilateral solver -------------------------------------------------------------------------------------------------------
static bool pcg_args_ok(const int32_t* neighbours, int32_t d, int64_t v, int32_t pitch, const void* a, const void* b) {
  return neighbours && d >= 1 && d <= kLtAxes - 1 && v >= 1 && feature_args_ok(v, pitch, a, b) && a && b;
}

struct PcgPasses {  // the grid's default blur: per axis y = b x + (c b) x[fwd], then y + a y[bwd]
  float s0[2], s1[2];
};

// A p into `Ap`, the partials of sum p . A p into `partial`; `spare`: two [v, pitch] buffers.  Returns the number of partials.
static int pcg_matvec(const int32_t* nb, int d, int64_t v, int P4, const PcgPasses& ps, const float* nvec, const float* dc,
                      float lam, const float* p, float* spare, const double* skip, float* Ap, double* partial, hipStream_t s) {
  const int L = row_lanes(P4);
  const dim3 grid(capped_grid(ceil_div(v, kRowThreads / L))), block(kRowThreads);
  float4* buf[2] = {(float4*)spare, (float4*)spare + v * P4};
  hipLaunchKernelGGL(lt_blur_scaled_kernel, grid, block, 0, s, (const float4*)p, nvec, nb, ps.s0[0], ps.s1[0], v, P4, L, skip,
                     buf[0]);
  for (int i = 1; i < 2 * d - 1; ++i)
    hipLaunchKernelGGL(lt_blur_kernel, grid, block, 0, s, (const float4*)buf[(i - 1) & 1], nb + (int64_t)i * v,
                       (const int32_t*)nullptr, ps.s0[i & 1], ps.s1[i & 1], 0.f, v, P4, L, buf[i & 1]);
  const int last = 2 * d - 1;
  hipLaunchKernelGGL(lt_matvec_last_kernel, grid, block, 0, s, (const float4*)buf[(last - 1) & 1], nb + (int64_t)last * v,
                     ps.s0[1], ps.s1[1], (const float4*)p, nvec, dc, lam, v, P4, L, skip, (float4*)Ap, partial);
  return (int)grid.x;
}

static PcgPasses pcg_passes(float tap_a, float tap_b, float tap_c) {
  return PcgPasses{{tap_b, 1.f}, {(float)((double)tap_c * (double)tap_b), tap_a}};
}

int32_t wcn_lattice_max_grid(void) { return kRowMaxGrid; }

int32_t wcn_lattice_row_grid(int64_t rows, int32_t pitch) {
  if (rows < 0 || pitch < 4 || pitch % 4 != 0) return 0;
  return (int32_t)capped_grid(ceil_div(rows, kRowThreads / row_lanes(pitch / 4)));
}

int wcn_bilateral_matvec(const int32_t* neighbours, int32_t d, int64_t v, int32_t pitch, float tap_a, float tap_b, float tap_c,
                         const float* nvec, const float* dc, float lam, const float* p, float* spare, float* ap,
                         double* partials, wcn_stream_t stream) {
  if (v == 0) return WCN_SUCCESS;
  if (!pcg_args_ok(neighbours, d, v, pitch, p, ap) || !nvec || !dc || !spare || !partials || !aligned_to(spare, 16) || p == ap)
    return WCN_ERROR_INVALID_PARAMETERS;
  pcg_matvec(neighbours, d, v, pitch / 4, pcg_passes(tap_a, tap_b, tap_c), nvec, dc, lam, p, spare, nullptr, ap, partials,
             (hipStream_t)stream);
  return launch_status();
}

int wcn_bilateral_pcg(const int32_t* neighbours, int32_t d, int64_t v, int32_t pitch, float tap_a, float tap_b, float tap_c,
                      const float* nvec, const float* dc, const float* minv, float lam, const float* tbar, float* y, float* work,
                      double* partials, double* state, int32_t max_iters, double tol, wcn_stream_t stream) {
  if (max_iters < 0 || !state) return WCN_ERROR_INVALID_PARAMETERS;
  if (v == 0) return WCN_SUCCESS;
  if (!pcg_args_ok(neighbours, d, v, pitch, tbar, y) || !nvec || !dc || !minv || !work || !partials || !aligned_to(work, 16) ||
      tbar == y)
    return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  const int P4 = pitch / 4, L = row_lanes(P4);
  const int64_t rows = v * pitch;  // floats of one buffer
  float *r = work, *p = work + rows, *z = work + 2 * rows, *ap = work + 3 * rows, *spare = work + 4 * rows;
  double *pap_part = partials, *rr_part = partials + kRowMaxGrid, *rz_part = partials + 2 * kRowMaxGrid;
  const PcgPasses ps = pcg_passes(tap_a, tap_b, tap_c);
  const dim3 block(kRowThreads);
  // the first residual: A y0 through the same matvec, then r, z, p and the state block
  const int parts = pcg_matvec(neighbours, d, v, P4, ps, nvec, dc, lam, y, spare, nullptr, ap, pap_part, s);
  const dim3 grid(parts);
  hipLaunchKernelGGL(lt_pcg_update_kernel<true>, grid, block, 0, s, (const double*)state, 0, (const double*)pap_part, parts,
                     (float4*)p, (const float4*)ap, minv, (const float4*)tbar, (float4*)y, (float4*)r, (float4*)z, v, P4, L,
                     rr_part, rz_part);
  hipLaunchKernelGGL(lt_pcg_start_kernel, dim3(1), block, 0, s, state, (const double*)rr_part, (const double*)rz_part, parts);
  for (int it = 0; it < max_iters; ++it) {  // 2 d + 2 launches, no host read
    pcg_matvec(neighbours, d, v, P4, ps, nvec, dc, lam, p, spare, state + kPcgDone + (it & 1), ap, pap_part, s);
    hipLaunchKernelGGL(lt_pcg_update_kernel<false>, grid, block, 0, s, (const double*)state, it, (const double*)pap_part, parts,
                       (float4*)p, (const float4*)ap, minv, (const float4*)tbar, (float4*)y, (float4*)r, (float4*)z, v, P4, L,
                       rr_part, rz_part);
    hipLaunchKernelGGL(lt_pcg_direction_kernel, grid, block, 0, s, state, it, tol, (const double*)rr_part,
                       (const double*)rz_part, parts, (const float4*)z, (float4*)p, v, P4, L);
  }
  return launch_status();
}

int wcn_bilateral_knn_weights(const float* src_xyz, const float* src_feat, const float* query_xyz, const float* query_feat,
                              const int64_t* nbr, int64_t n, int64_t m, int32_t k, int32_t dx, int32_t df, float sigma_xyz,
                              float sigma_feat, float* weights, wcn_stream_t stream) {
  if (n < 0 || m < 0 || k < 1 || dx < 1 || df < 1 || n > INT32_MAX || m * (int64_t)k > INT32_MAX || !(sigma_xyz > 0.f) ||
      !(sigma_feat > 0.f))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (m == 0) return WCN_SUCCESS;
  if (!query_xyz || !query_feat || !nbr || !weights || (n > 0 && (!src_xyz || !src_feat))) return WCN_ERROR_INVALID_PARAMETERS;
  const float inv_xyz = (float)(1.0 / (2.0 * (double)sigma_xyz * (double)sigma_xyz));
  const float inv_feat = (float)(1.0 / (2.0 * (double)sigma_feat * (double)sigma_feat));
  hipLaunchKernelGGL(bilateral_knn_weights_kernel, dim3(capped_grid(ceil_div(m, kRowThreads))), dim3(kRowThreads), 0,
                     (hipStream_t)stream, src_xyz, src_feat, query_xyz, query_feat, nbr, n, m, (int)k, (int)dx, (int)df,
                     inv_xyz, inv_feat, weights);
  return launch_status();
}

}  // extern "C"
