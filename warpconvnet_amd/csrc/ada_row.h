// ada_row.h - the row helpers of the row-streaming norm kernels (adaln.hip, ln_act.hip): a row of C channels is C / 8 pieces
// of 8 elements (one 16-B access of f16 / bf16, two of f32); G = the power of two >= min(C / 8, 64) lanes stand side by side
// on a row and hold it in registers, up to 4 pieces each; sums over a row cross its G lanes with an xor butterfly.
#pragma once

#include "wcn_common.h"

namespace wcn {

constexpr int kAdaThreads = 256;
constexpr int kAdaChunk = 64;        // rows of one backward chunk
constexpr int kAdaMaxChannels = 2048;
constexpr int kAdaFwdBlocks = 4096;  // the forward's grid is capped here; its lane groups stride over the rows

template <typename T> struct alignas(16) AdaVec8 { T v[8]; };

template <typename T>
__device__ __forceinline__ void ada_ld8(const T* __restrict__ p, float (&f)[8]) {
  if constexpr (sizeof(T) == 4) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  } else {
    const AdaVec8<T> v = *reinterpret_cast<const AdaVec8<T>*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (float)v.v[e];
  }
}

template <typename T>
__device__ __forceinline__ void ada_st8(T* __restrict__ p, const float (&f)[8]) {
  if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
  } else {
    AdaVec8<T> v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v.v[e] = (T)f[e];
    *reinterpret_cast<AdaVec8<T>*>(p) = v;
  }
}

// sum over the G = 1 << glog lanes of a group; every lane of the group receives the same bits
__device__ __forceinline__ float ada_group_sum(float v, int glog) {
  for (int m = 0; m < glog; ++m) v += __shfl_xor(v, 1 << m);
  return v;
}

}  // namespace wcn
