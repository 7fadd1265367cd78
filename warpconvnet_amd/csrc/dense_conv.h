// dense_conv.h - what the dense convolutions on channels-last rows share (internal): dense_conv3d.hip (bricks) and
// dense_conv2d.hip (image tiles).  The fragment step of one MFMA pair per dtype, the zero-padded 16-B row pieces, the staged
// tiles of the weight gradient with their K-major reads, its bias-gradient and ordered-reduce kernels and the slab plan.
#pragma once

#include "gather_gemm.h"

namespace wcn {

constexpr int kDcThreads = 256;
constexpr int kDwTile = 64;                     // weight gradient: channels per block on both sides
constexpr int kDwBiasParts = 64;                // row ranges of the bias gradient
constexpr int kDwTargetGroups = 1024;           // workgroups the slab count aims at (four per CU)
constexpr int kDwMaxSlabs = 256;

typedef __attribute__((ext_vector_type(4))) short dc_s16x4;

// One reduction step of a fragment pair: every lane brings 16 B of its row (A) / column (B), k = E * (lane / 32) + e.
template <typename T> struct DcOp {
  static constexpr int E = 8;
  static __device__ __forceinline__ f32x16 mma(const Vec<T, 8>& a, const Vec<T, 8>& b, f32x16 c) {
    typedef typename Mfma32<T>::type F;
    return Mfma32<T>::mfma(__builtin_bit_cast(F, a), __builtin_bit_cast(F, b), c);
  }
};
template <> struct DcOp<float> {
  static constexpr int E = 4;  // four 32x32x2 products, product e takes element e of every lane
  static __device__ __forceinline__ f32x16 mma(const Vec<float, 4>& a, const Vec<float, 4>& b, f32x16 c) {
#pragma unroll
    for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[e], b.v[e], c, 0, 0, 0);
    return c;
  }
};

template <typename T, int E>
__device__ __forceinline__ Vec<T, E> dc_zero() {
  Vec<T, E> v;
#pragma unroll
  for (int e = 0; e < E; ++e) v.v[e] = (T)0.f;
  return v;
}

// channels [k0, k0 + E) of a row of `c` channels, zeros past the end; `vec`: c % E == 0 and the tensor is 16-B aligned
template <typename T, int E>
__device__ __forceinline__ Vec<T, E> dc_load_piece(const T* __restrict__ row, int k0, int c, int vec) {
  Vec<T, E> v = dc_zero<T, E>();
  if (k0 >= c) return v;
  if (vec) return *reinterpret_cast<const Vec<T, E>*>(row + k0);
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (k0 + e < c) v.v[e] = row[k0 + e];
  return v;
}

// ---- weight gradient: staged tiles --------------------------------------------------------------------------------------------
template <typename T> struct DwTile {
  static constexpr int E = DcOp<T>::E;
  static constexpr int VSTEP = sizeof(T) == 2 ? 128 : 64;                  // rows (voxels / pixels) of one step
  static constexpr int PPR = kDwTile / E;                                   // 16-B pieces of a staged row
  static constexpr int PITCH = kDwTile * (int)sizeof(T) + (sizeof(T) == 2 ? 0 : 16);
  static constexpr int BYTES = VSTEP * PITCH;
  static constexpr int PER = VSTEP * PPR / kDcThreads;                      // pieces a thread brings per tile and step
  static_assert(PER == 4, "1024 pieces per tile");
};

// where piece `c` of staged row `p` lives: the 16-bit tiles carry the chunk swizzle the transpose read expects
template <typename T>
__device__ __forceinline__ int dw_piece_at(int p, int c) {
  if (sizeof(T) == 2) return p * DwTile<T>::PITCH + ((c ^ (((p >> 1) & 1) << 2)) << 4);
  return p * DwTile<T>::PITCH + (c << 4);
}

// 16-bit fragment for MFMA rows / columns [c0, c0 + 32) and rows [p0, p0 + 16): lane (h, m) gets tile[p0 + 8h + j][c0 + m]
template <typename T>
__device__ __forceinline__ Vec<T, 8> dw_read_tr(const char* tile, int p0, int c0, int lane) {
  const int g = lane >> 4, i = lane & 15;
  const int col = c0 + 16 * (g & 1) + 4 * (i & 3);
  Vec<T, 8> out;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int p = p0 + 8 * (g >> 1) + 4 * t + (i >> 2);
    const char* addr = tile + dw_piece_at<T>(p, col >> 3) + (col & 7) * 2;
    const dc_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((dc_s16x4 __attribute__((address_space(3)))*)addr);
#pragma unroll
    for (int e = 0; e < 4; ++e) out.v[4 * t + e] = __builtin_bit_cast(T, (short)v[e]);
  }
  return out;
}

// one step of the staged tiles: acc += s_x[:, 32 wi ..]^T s_y[:, 32 wj ..] over the VSTEP rows
template <typename T>
__device__ __forceinline__ f32x16 dw_step_mma(const char* s_x, const char* s_y, int wi, int wj, int lane, f32x16 acc) {
  typedef DwTile<T> TL;
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int p0 = 0; p0 < TL::VSTEP; p0 += 16)
      acc = DcOp<T>::mma(dw_read_tr<T>(s_x, p0, 32 * wi, lane), dw_read_tr<T>(s_y, p0, 32 * wj, lane), acc);
  } else {
    const int half = lane >> 5, r = lane & 31;
#pragma unroll 8
    for (int p0 = 0; p0 < TL::VSTEP; p0 += 2) {
      const float a = *reinterpret_cast<const float*>(s_x + (p0 + half) * TL::PITCH + (32 * wi + r) * 4);
      const float bq = *reinterpret_cast<const float*>(s_y + (p0 + half) * TL::PITCH + (32 * wj + r) * 4);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bq, acc, 0, 0, 0);
    }
  }
  return acc;
}

// bias gradient, first pass: bpart[g][c] = sum of rows[.][c] over row range g (rows in eight interleaved runs, added in run order)
template <typename T>
__global__ __launch_bounds__(kDcThreads) void dense_conv_dbias_kernel(const T* __restrict__ dy, float* __restrict__ bpart,
                                                                      int64_t nvox, int cout) {
  __shared__ float s_sum[8][32];
  const int rg = threadIdx.x >> 5, cl = threadIdx.x & 31;
  const int64_t per = (nvox + kDwBiasParts - 1) / kDwBiasParts;
  const int64_t r0 = blockIdx.x * per, r1 = r0 + per < nvox ? r0 + per : nvox;
  for (int c0 = 0; c0 < cout; c0 += 32) {
    const int c = c0 + cl;
    float s = 0.f;
    if (c < cout)
      for (int64_t row = r0 + rg; row < r1; row += 8) s += (float)dy[row * cout + c];
    s_sum[rg][cl] = s;
    __syncthreads();
    if (rg == 0 && c < cout) {
      float tot = s_sum[0][cl];
#pragma unroll
      for (int g = 1; g < 8; ++g) tot += s_sum[g][cl];
      bpart[(int64_t)blockIdx.x * cout + c] = tot;
    }
    __syncthreads();
  }
}

// dW [Cout, Cin, kv] = the slabs added in slab order, rounded once; dbias [nbias] = its parts added in order
template <typename T>
__global__ __launch_bounds__(kDcThreads) void dense_conv_wgrad_reduce_kernel(const float* __restrict__ part,
                                                                             const float* __restrict__ bpart, int slabs, int kv,
                                                                             int cin, int cout, int nbias, T* __restrict__ dw,
                                                                             T* __restrict__ dbias) {
  const int64_t cells = (int64_t)kv * cin * cout;
  const int64_t total = cells + (dbias ? nbias : 0);
  for (int64_t e = (int64_t)blockIdx.x * kDcThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kDcThreads) {
    float s = 0.f;
    if (e < cells) {
      for (int g = 0; g < slabs; ++g) s += part[g * cells + e];
      const int co = (int)(e % cout);
      const int64_t t = e / cout;
      const int ci = (int)(t % cin), delta = (int)(t / cin);
      dw[((int64_t)co * cin + ci) * kv + delta] = (T)s;
    } else {
      const int c = (int)(e - cells);
      for (int g = 0; g < kDwBiasParts; ++g) s += bpart[(int64_t)g * nbias + c];
      dbias[c] = (T)s;
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
static inline int dc_step(int dtype) { return 32 / dtype_bytes(dtype); }  // S: reduction elements of a fragment step
static inline int dc_round(int v, int m) { return (v + m - 1) / m * m; }
static inline int dc_nb(int n) { return n > 64 ? 2 : 1; }                 // 32-column blocks per wave
static inline int64_t dc_vstep(int dtype) { return dtype == WCN_F32 ? 64 : 128; }

// rows per slab (a multiple of the step) and the slabs that are not empty
static inline void dw_plan(int64_t nvox, int slabs, int dtype, int64_t* slab_vox, int* used) {
  const int64_t vs = dc_vstep(dtype);
  *slab_vox = ceil_div(ceil_div(nvox, slabs), vs) * vs;
  *used = (int)ceil_div(nvox, *slab_vox);
}

// the slab count of a weight gradient over `rows` rows and `kv` offsets: enough workgroups, no more slabs than steps
static inline int dw_slabs(int64_t rows, int cin, int cout, int kv, int dtype) {
  const int64_t groups = (int64_t)kv * ceil_div(cin, kDwTile) * ceil_div(cout, kDwTile);
  int64_t slabs = ceil_div(kDwTargetGroups, groups);
  const int64_t steps = ceil_div(rows, dc_vstep(dtype));
  if (slabs > steps) slabs = steps;
  if (slabs > kDwMaxSlabs) slabs = kDwMaxSlabs;
  return (int)slabs;
}

}  // namespace wcn
