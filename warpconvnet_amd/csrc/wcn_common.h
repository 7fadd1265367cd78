// wcn_common.h - shared device helpers for the gfx950 sparse-conv kernels.
//
// Key packing / hash follow the reference's published table format so that range errors and
// wrap-around behaviour are identical (reference: warpconvnet/csrc/include/cuhash/hash_functions.cuh:29-84).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/wcn.h"

namespace wcn {

constexpr int kBatchBits = 9;
constexpr int kCoordBits = 18;
constexpr uint32_t kBatchMask = (1u << kBatchBits) - 1;  // 0x1FF
constexpr uint32_t kCoordMask = (1u << kCoordBits) - 1;  // 0x3FFFF
constexpr int kCoordMax = (1 << (kCoordBits - 1)) - 1;   // 131071
constexpr int kCoordMin = -(1 << (kCoordBits - 1));      // -131072
constexpr int kBatchMax = (1 << kBatchBits) - 1;         // 511
constexpr uint64_t kValidBit = 1ull << 63;

// 16-byte hash slot: one dwordx4 load returns key and value together.
struct __attribute__((aligned(16))) Slot {
  uint64_t key;    // 0 = empty
  int32_t value;   // row index (smallest among duplicates); -1 while empty
  int32_t pad;
};

__host__ __device__ __forceinline__ uint64_t pack_key(int b, int x, int y, int z) {
  return kValidBit | ((uint64_t)((uint32_t)b & kBatchMask) << 54) | ((uint64_t)((uint32_t)x & kCoordMask) << 36) |
         ((uint64_t)((uint32_t)y & kCoordMask) << 18) | (uint64_t)((uint32_t)z & kCoordMask);
}

// Splitmix64 finaliser, masked to the (power-of-two) capacity.
__host__ __device__ __forceinline__ uint32_t hash_slot(uint64_t key, uint32_t capacity_mask) {
  key ^= key >> 30;
  key *= 0xBF58476D1CE4E5B9ull;
  key ^= key >> 27;
  key *= 0x94D049BB133111EBull;
  key ^= key >> 31;
  return (uint32_t)key & capacity_mask;
}

__host__ __device__ __forceinline__ bool coord_in_range(int b, int x, int y, int z) {
  return b >= 0 && b <= kBatchMax && x >= kCoordMin && x <= kCoordMax && y >= kCoordMin && y <= kCoordMax &&
         z >= kCoordMin && z <= kCoordMax;
}

// Linear-probe lookup; returns the stored row index or -1.
__device__ __forceinline__ int slot_lookup(const Slot* __restrict__ slots, uint32_t capacity_mask, uint64_t key) {
  uint32_t s = hash_slot(key, capacity_mask);
  for (uint32_t attempts = 0; attempts <= capacity_mask; ++attempts) {
    const uint4 v = *reinterpret_cast<const uint4*>(slots + s);
    const uint64_t k = ((uint64_t)v.y << 32) | v.x;
    if (k == 0ull) return -1;
    if (k == key) return (int)v.z;
    s = (s + 1) & capacity_mask;
  }
  return -1;
}

// LDS-DMA issued through inline asm: hipcc neither counts these in its own s_waitcnt bookkeeping nor orders
// later LDS reads behind them (with the builtin it drains vmcnt(0) before the first ds_read of every step, which
// serialises the ring).  Completion is tracked by the counted s_waitcnt vmcnt(N) below.  M0 (LDS destination base)
// is written and restored inside the statement; `lds_addr` must be wave-uniform.
__device__ __forceinline__ uint32_t lds_addr_of(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}
__device__ __forceinline__ void glds16(const void* gsrc, uint32_t lds_addr) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_addr)
               : "memory");
}
__device__ __forceinline__ void glds4(const void* gsrc, uint32_t lds_addr) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_addr)
               : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

inline int launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? WCN_SUCCESS : WCN_ERROR_KERNEL_EXECUTION;
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline bool valid_k(int64_t num_offsets) { return num_offsets >= 1 && num_offsets <= 4096; }  // kernel volumes the library takes

// ---- elements ------------------------------------------------------------------------------------------------------------
// The one convention: a storage dtype (WCN_F32 / WCN_F16 / WCN_BF16) is float / _Float16 / __bf16 - the types the MFMA
// fragments take - and becomes a float, and a float it, by a C cast (round to nearest even).

// N elements moved as one access
template <typename T, int N> struct alignas(sizeof(T) * N) Vec { T v[N]; };

// V elements at p <-> floats: one access of sizeof(T) * V bytes up to 16, beyond that 16-B pieces in ascending order
template <typename T, int V>
__device__ __forceinline__ void ld_vec(const T* __restrict__ p, float (&f)[V]) {
  constexpr int P = sizeof(T) * V <= 16 ? V : 16 / (int)sizeof(T);
  static_assert(V % P == 0, "whole pieces");
#pragma unroll
  for (int i = 0; i < V; i += P) {
    const Vec<T, P> v = *reinterpret_cast<const Vec<T, P>*>(p + i);
#pragma unroll
    for (int e = 0; e < P; ++e) f[i + e] = (float)v.v[e];
  }
}
template <typename T, int V>
__device__ __forceinline__ void st_vec(T* __restrict__ p, const float (&f)[V]) {
  constexpr int P = sizeof(T) * V <= 16 ? V : 16 / (int)sizeof(T);
  static_assert(V % P == 0, "whole pieces");
#pragma unroll
  for (int i = 0; i < V; i += P) {
    Vec<T, P> v;
#pragma unroll
    for (int e = 0; e < P; ++e) v.v[e] = (T)f[i + e];
    *reinterpret_cast<Vec<T, P>*>(p + i) = v;
  }
}

inline bool dtype_ok(int dtype) { return dtype == WCN_F32 || dtype == WCN_F16 || dtype == WCN_BF16; }
inline int dtype_bytes(int dtype) { return dtype == WCN_F32 ? 4 : 2; }

// f(T{}) for the element type of a dtype code (dtype_ok); with_dtype16 where the caller has ruled out WCN_F32
template <typename F>
inline int with_dtype(int dtype, F&& f) {
  return dtype == WCN_F32 ? f(float{}) : dtype == WCN_F16 ? f(_Float16{}) : f(__bf16{});
}
template <typename F>
inline int with_dtype16(int dtype, F&& f) {
  return dtype == WCN_F16 ? f(_Float16{}) : f(__bf16{});
}

// f(T{}, std::integral_constant<int, V>{}) for the dtype and a piece of `vec` elements: a 16-B piece, half of one (only
// with HALF) or, for every other `vec`, one element
template <bool HALF, typename F>
inline int with_dtype_vec(int dtype, int vec, F&& f) {
  return with_dtype(dtype, [&](auto t) {
    constexpr int W = 16 / (int)sizeof(t);
    if (vec == W) return f(t, std::integral_constant<int, W>{});
    if constexpr (HALF)
      if (vec == W / 2) return f(t, std::integral_constant<int, W / 2>{});
    return f(t, std::integral_constant<int, 1>{});
  });
}

// a = a power of two; true for null (an absent optional buffer)
inline bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// ---- prefix sums (wave64) -------------------------------------------------------------------------------------------------
// inclusive scan over the first WIDTH (64 or 32) lanes of a wave; with 32 the upper half's results are unspecified
template <int WIDTH = 64>
__device__ __forceinline__ int wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < WIDTH; d <<= 1) {
    const int up = __shfl_up(v, d);
    if (lane >= d) v += up;
  }
  return v;
}

// exclusive scan of one int per thread over a workgroup of THREADS; *total = the workgroup's sum (all threads).  `s_wave`:
// THREADS / 64 ints of LDS - the caller puts a barrier in front of its next use
template <int THREADS>
__device__ __forceinline__ int block_excl_scan(int v, int* s_wave, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = wave_incl_scan(v);
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    const int q = s_wave[w];
    if (w < wave) base += q;
    tot += q;
  }
  *total = tot;
  return base + incl - v;
}

// exclusive scan of n counts in place by ONE workgroup of THREADS, THREADS * PER counts a trip; returns their sum (all
// threads).  16-B accesses: `counts` is 16-B aligned and n a multiple of 4 (a lane-strided 4-B access costs one
// texture-addresser slot per lane and element).
template <int THREADS, int PER>
__device__ __forceinline__ int scan_counts_in_place(int32_t* __restrict__ counts, int64_t n, int* s_wave) {
  static_assert(PER % 4 == 0, "whole int4 pieces");
  int carry = 0;
  for (int64_t base = 0; base < n; base += THREADS * PER) {
    const int64_t i0 = base + (int64_t)threadIdx.x * PER;
    int v[PER];
    int sum = 0;
#pragma unroll
    for (int j = 0; j < PER; j += 4) {
      int4 q = make_int4(0, 0, 0, 0);
      if (i0 + j < n) q = *reinterpret_cast<const int4*>(counts + i0 + j);
      v[j] = q.x; v[j + 1] = q.y; v[j + 2] = q.z; v[j + 3] = q.w;
      sum += q.x + q.y + q.z + q.w;
    }
    int trip;
    int run = carry + block_excl_scan<THREADS>(sum, s_wave, &trip);
#pragma unroll
    for (int j = 0; j < PER; j += 4) {
      int4 q;
      q.x = run; run += v[j];
      q.y = run; run += v[j + 1];
      q.z = run; run += v[j + 2];
      q.w = run; run += v[j + 3];
      if (i0 + j < n) *reinterpret_cast<int4*>(counts + i0 + j) = q;
    }
    carry += trip;
    __syncthreads();  // s_wave is rewritten by the next trip
  }
  return carry;
}

// ---- bisections -----------------------------------------------------------------------------------------------------------
// first row whose batch index (coords[.].x) is >= b; rows are batch-sorted
__device__ __forceinline__ int64_t first_row_of_batch(const int4* __restrict__ coords, int64_t n, int b) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (coords[mid].x < b) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// largest k in [0, K) with offsets[k] <= p (offsets ascending, offsets[0] <= p; K = 1 reads nothing)
__device__ __forceinline__ int last_offset_not_above(const int32_t* __restrict__ offsets, int K, int64_t p) {
  int lo = 0, hi = K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// Per-device one-time setup (kernel attributes are per device context): bit d of `done` = device d is set up.  The only
// process-wide state of the library, idempotent: a lost race or a device index above 63 just repeats the setup call.
template <typename F>
inline int once_per_device(unsigned long long& done, F&& setup) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return WCN_ERROR_KERNEL_INITIALIZATION;
  if (dev >= 0 && dev < 64 && ((__atomic_load_n(&done, __ATOMIC_RELAXED) >> dev) & 1ull)) return WCN_SUCCESS;
  if (!setup()) return WCN_ERROR_KERNEL_INITIALIZATION;
  if (dev >= 0 && dev < 64) __atomic_fetch_or(&done, 1ull << dev, __ATOMIC_RELAXED);
  return WCN_SUCCESS;
}

// Epilogue of the gather GEMM, applied in fp32 before the result is rounded to the storage dtype:
//   y = act((acc + bias) * scale + shift + residual)      every term optional (null / 0 = absent)
// BatchNorm in inference mode is scale = gamma / sqrt(var + eps), shift = beta - mean * scale.
struct ConvEpilogue {
  const float* bias = nullptr;     // [cout]
  const float* scale = nullptr;    // [cout], used together with shift
  const float* shift = nullptr;    // [cout]
  const void* residual = nullptr;  // [n_out][cout] in the storage dtype
  int relu = 0;
};

}  // namespace wcn
