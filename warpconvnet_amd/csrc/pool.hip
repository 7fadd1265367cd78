// pool.hip - sparse pooling over a kernel map (REDUCE_AND_STRIDE and the SparsePool modules).
//
//   wcn_pool_gather  out[m][c] = reduce_k in[tbl[m][k]][c]   reduce in {sum, mean, max, min}; rows of `tbl` with no
//                    neighbour give zero; max / min also return the winning input row (first extremum in offset
//                    order) for the backward pass, and the neighbour count per row on request.
//   wcn_pool_gather_scaled  the same with in[r][c] * scale[r] (fp32, per SOURCE row) in place of in[r][c]: the backward of
//                    the mean, whose terms dy[r] / count[r] are formed and summed in fp32 and rounded once.
//   wcn_pool_select  dx[n][c] = sum_k [arg[tbl[n][k]][c] == n] * dy[tbl[n][k]][c]   - gradient of max / min pooling,
//                    output-stationary over the REVERSE table (deterministic, no atomics).
//
// Both walk the row-major neighbour table the convolution kernels use ([rows][kp] int32, -1 = absent).  Adjacent lanes
// hold adjacent 16-B pieces of one feature row, so every neighbour access is a whole-row (coalesced) read; fp32
// accumulation.  The 16-B pieces need 16-B aligned feature pointers (a contiguous view may start anywhere in its
// storage): the host checks them and takes the one-element path otherwise.  The reference runs this as to_csr (a device sort) + feature gather + torch_scatter.segment_csr
// (warpconvnet/nn/functional/sparse_pool.py:84-110); here it is one pass over the table with no intermediate tensor.

#include <cfloat>

#include "wcn_common.h"

namespace wcn {

enum { kPoolSum = 0, kPoolMean = 1, kPoolMax = 2, kPoolMin = 3 };

template <typename T, int VEC>
__global__ __launch_bounds__(256) void pool_gather_kernel(const T* __restrict__ in, const int32_t* __restrict__ tbl,
                                                          const float* __restrict__ scale, int64_t m, int c, int K,
                                                          int kp, int op, T* __restrict__ out,
                                                          int32_t* __restrict__ arg, int32_t* __restrict__ count) {
  const int cv = c / VEC;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m * cv) return;
  const int64_t row = idx / cv;
  const int v = (int)(idx % cv);
  float acc[VEC];
  int32_t best[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) { acc[j] = 0.f; best[j] = -1; }
  int n = 0;
  const int32_t* trow = tbl + row * kp;
  for (int k = 0; k < K; ++k) {
    const int32_t r = trow[k];
    if (r < 0) continue;
    const Vec<T, VEC> x = *reinterpret_cast<const Vec<T, VEC>*>(in + (int64_t)r * c + (int64_t)v * VEC);
    const float sc = scale ? scale[r] : 1.0f;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float f = (float)x.v[j] * sc;
      asm volatile("" : "+v"(f));  // (the same: the scaled term is an fp32 number in both instantiations, never an fma operand)
      if (op == kPoolMax) { if (n == 0 || f > acc[j]) { acc[j] = f; best[j] = r; } }
      else if (op == kPoolMin) { if (n == 0 || f < acc[j]) { acc[j] = f; best[j] = r; } }
      else acc[j] += f;
    }
    ++n;
  }
  Vec<T, VEC> y;
  const float inv = (op == kPoolMean && n > 0) ? 1.0f / (float)n : 1.0f;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    // the fp32 product is materialised before it is rounded to the storage type (the barrier of norm.hip's bn_affine): the
    // one-element fp16 instantiation otherwise fuses product and conversion into v_fma_mixlo_f16 (one rounding) while the
    // 16-B one multiplies and converts (two), and the same rows give other bits through a view that is not 16-B aligned
    float p = acc[j] * inv;
    asm volatile("" : "+v"(p));
    y.v[j] = (T)p;
  }
  *reinterpret_cast<Vec<T, VEC>*>(out + row * c + (int64_t)v * VEC) = y;
  if (arg) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) arg[row * c + (int64_t)v * VEC + j] = best[j];
  }
  if (count && v == 0) count[row] = n;
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void pool_select_kernel(const T* __restrict__ dy, const int32_t* __restrict__ arg,
                                                          const int32_t* __restrict__ tbl, int64_t n_rows, int c, int K,
                                                          int kp, T* __restrict__ dx) {
  const int cv = c / VEC;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_rows * cv) return;
  const int64_t row = idx / cv;
  const int v = (int)(idx % cv);
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
  const int32_t* trow = tbl + row * kp;
  for (int k = 0; k < K; ++k) {
    const int32_t r = trow[k];
    if (r < 0) continue;
    const int64_t at = (int64_t)r * c + (int64_t)v * VEC;
    const Vec<T, VEC> g = *reinterpret_cast<const Vec<T, VEC>*>(dy + at);
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      if (arg[at + j] == (int32_t)row) acc[j] += (float)g.v[j];
  }
  Vec<T, VEC> y;
#pragma unroll
  for (int j = 0; j < VEC; ++j) y.v[j] = (T)acc[j];
  *reinterpret_cast<Vec<T, VEC>*>(dx + row * c + (int64_t)v * VEC) = y;
}

// elements per access of a row kernel over the feature pointers a and b: a 16-B piece when the row is a whole number of
// pieces and both pointers are 16-B aligned (rows then stay aligned: c * sizeof(T) is a multiple of 16), else one element
template <typename T>
static int pool_row_vec(const void* a, const void* b, int c) {
  constexpr int VEC = 16 / (int)sizeof(T);
  return (c % VEC == 0 && aligned_to(a, 16) && aligned_to(b, 16)) ? VEC : 1;
}

template <typename T>
static int pool_gather_t(const void* in, const int32_t* tbl, const float* scale, int64_t m, int c, int K, int kp, int op,
                         void* out, int32_t* arg, int32_t* count, hipStream_t s) {
  constexpr int VEC = 16 / (int)sizeof(T);
  if (pool_row_vec<T>(in, out, c) == VEC) {
    hipLaunchKernelGGL((pool_gather_kernel<T, VEC>), dim3((unsigned)ceil_div(m * (c / VEC), 256)), dim3(256), 0, s,
                       (const T*)in, tbl, scale, m, c, K, kp, op, (T*)out, arg, count);
  } else {
    hipLaunchKernelGGL((pool_gather_kernel<T, 1>), dim3((unsigned)ceil_div(m * c, 256)), dim3(256), 0, s, (const T*)in, tbl,
                       scale, m, c, K, kp, op, (T*)out, arg, count);
  }
  return launch_status();
}

template <typename T>
static int pool_select_t(const void* dy, const int32_t* arg, const int32_t* tbl, int64_t n, int c, int K, int kp,
                         void* dx, hipStream_t s) {
  constexpr int VEC = 16 / (int)sizeof(T);
  if (pool_row_vec<T>(dy, dx, c) == VEC) {
    hipLaunchKernelGGL((pool_select_kernel<T, VEC>), dim3((unsigned)ceil_div(n * (c / VEC), 256)), dim3(256), 0, s,
                       (const T*)dy, arg, tbl, n, c, K, kp, (T*)dx);
  } else {
    hipLaunchKernelGGL((pool_select_kernel<T, 1>), dim3((unsigned)ceil_div(n * c, 256)), dim3(256), 0, s, (const T*)dy, arg,
                       tbl, n, c, K, kp, (T*)dx);
  }
  return launch_status();
}

}  // namespace wcn

using namespace wcn;

extern "C" {

int wcn_pool_row_vec(const void* src, const void* dst, int32_t channels, int32_t dtype) {
  if (channels < 1 || !dtype_ok(dtype)) return 0;
  return with_dtype(dtype, [&](auto t) { return pool_row_vec<decltype(t)>(src, dst, channels); });
}

int wcn_pool_gather_scaled(const void* in, const int32_t* tbl, const float* scale, int64_t n_in, int64_t n_out,
                           int32_t channels, int32_t num_offsets, int32_t dtype, int32_t op, void* out, int32_t* arg,
                           int32_t* count, wcn_stream_t stream) {
  if (n_in < 0 || n_out < 0 || channels < 0 || num_offsets < 1 || num_offsets > 4096 || op < kPoolSum || op > kPoolMin)
    return WCN_ERROR_INVALID_PARAMETERS;
  if (n_out == 0 || channels == 0) return WCN_SUCCESS;
  if (!tbl || !out || (n_in > 0 && !in)) return WCN_ERROR_INVALID_PARAMETERS;
  const int kp = wcn_kmap_row_pitch(num_offsets);
  hipStream_t s = (hipStream_t)stream;
  if (!dtype_ok(dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  const int el = dtype == WCN_F32 ? 4 : 2;
  if (!aligned_to(in, el) || !aligned_to(out, el) || !aligned_to(scale, 4)) return WCN_ERROR_INVALID_PARAMETERS;
  return with_dtype(dtype, [&](auto t) {
    return pool_gather_t<decltype(t)>(in, tbl, scale, n_out, channels, num_offsets, kp, op, out, arg, count, s);
  });
}

int wcn_pool_gather(const void* in, const int32_t* tbl, int64_t n_in, int64_t n_out, int32_t channels, int32_t num_offsets,
                    int32_t dtype, int32_t op, void* out, int32_t* arg, int32_t* count, wcn_stream_t stream) {
  return wcn_pool_gather_scaled(in, tbl, nullptr, n_in, n_out, channels, num_offsets, dtype, op, out, arg, count, stream);
}

int wcn_pool_select(const void* dy, const int32_t* arg, const int32_t* tbl, int64_t n_in, int64_t n_out, int32_t channels,
                    int32_t num_offsets, int32_t dtype, void* dx, wcn_stream_t stream) {
  if (n_in < 0 || n_out < 0 || channels < 0 || num_offsets < 1 || num_offsets > 4096) return WCN_ERROR_INVALID_PARAMETERS;
  if (n_in == 0 || channels == 0) return WCN_SUCCESS;
  if (!tbl || !dx || (n_out > 0 && (!dy || !arg))) return WCN_ERROR_INVALID_PARAMETERS;
  const int kp = wcn_kmap_row_pitch(num_offsets);
  hipStream_t s = (hipStream_t)stream;
  if (!dtype_ok(dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  const int el = dtype == WCN_F32 ? 4 : 2;
  if (!aligned_to(dy, el) || !aligned_to(dx, el)) return WCN_ERROR_INVALID_PARAMETERS;
  return with_dtype(dtype, [&](auto t) {
    return pool_select_t<decltype(t)>(dy, arg, tbl, n_in, channels, num_offsets, kp, dx, s);
  });
}

}  // extern "C"
