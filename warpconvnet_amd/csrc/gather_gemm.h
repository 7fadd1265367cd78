// gather_gemm.h - what the three forward / dgrad gather-GEMM families share (internal):
//   conv_mfma.hip     32x32x16, rows gathered into registers, weights by LDS-DMA (also groups, K > 32)
//   conv_mfma16.hip   16x16x32, same structure, the channel counts the others do not take
//   conv_mfma_cs.hip  channel-split, rows staged through LDS (the headline shapes)
// Every piece here is used as it is by at least two of them; what one family alone needs stays in its file.  The
// prototypes at the end are the only declarations of the functions these files and conv_api.hip call across
// translation units.
#pragma once

#include "wcn_common.h"

namespace wcn {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// One trait per matrix-core shape: operand fragment type (8 values of T per lane) and the instruction.
template <typename T> struct Mfma32;  // v_mfma_f32_32x32x16: 16 fp32 results per lane
template <> struct Mfma32<__bf16> {
  typedef bf16x8 type;
  static __device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct Mfma32<_Float16> {
  typedef f16x8 type;
  static __device__ __forceinline__ f32x16 mfma(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};
template <typename T> struct Mfma16;  // v_mfma_f32_16x16x32: 4 fp32 results per lane
template <> struct Mfma16<__bf16> {
  typedef bf16x8 type;
  static __device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct Mfma16<_Float16> {
  typedef f16x8 type;
  static __device__ __forceinline__ f32x4 mfma(f16x8 a, f16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};

// ---- tile prologue ---------------------------------------------------------------------------------------------------
// Output rows of the tile through the mask-sorted permutation (-1 past the end).  The caller's barrier publishes them.
template <int TILE>
__device__ __forceinline__ void stage_row_ids(int32_t* s_rows, const int32_t* perm, int64_t row0, int64_t n_out) {
  const int tid = threadIdx.x;
  if (tid < TILE) {
    const int64_t pr = row0 + tid;
    int32_t r = -1;
    if (pr < n_out) r = perm ? perm[pr] : (int32_t)pr;
    s_rows[tid] = r;
  }
}

// OR of the row masks per block of BLK rows (s_wmask zeroed and published by the caller): a wave skips the MFMAs of a
// row block none of whose rows has the offset.  Thread tid brings the mask of tile row tid.
template <int TILE, int BLK>
__device__ __forceinline__ void or_row_mask(uint32_t* s_wmask, uint32_t my_mask) {
  const int tid = threadIdx.x;
  if (tid < TILE && my_mask) atomicOr(&s_wmask[tid / BLK], my_mask);
}
// offsets any row of the tile has (wave-uniform: an SGPR)
template <int NBLK>
__device__ __forceinline__ uint32_t tile_mask(const uint32_t* s_wmask) {
  uint32_t m = 0u;
#pragma unroll
  for (int q = 0; q < NBLK; ++q) m |= s_wmask[q];
  return __builtin_amdgcn_readfirstlane(m);
}

// ---- step loop -------------------------------------------------------------------------------------------------------
// step iterator over (set bits of the tile's mask ascending) x (channel chunks); start with k = -1
struct StepIter {
  uint32_t rem;
  int nchunk;
  __device__ __forceinline__ bool next(int& k, int& chunk) {
    if (k >= 0 && chunk + 1 < nchunk) { ++chunk; return true; }
    if (rem == 0u) return false;
    k = __builtin_ctz(rem);
    rem &= rem - 1u;
    chunk = 0;
    return true;
  }
};

// LDS-DMA completion is tracked by vmcnt; drain it explicitly before every barrier.  The BUILTIN, not an asm statement:
// it also resets hipcc's own load scoreboard (see the header of conv_mfma.hip).
__device__ __forceinline__ void sync_step() {
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), gfx9 encoding
  __syncthreads();
}

// weight slab of one step, HBM -> LDS by LDS-DMA in the order the fragments are read back; the waves share the 1-KiB units
// wave / lane BY REFERENCE on purpose: by value the register allocation of the widest kernel moves (226 -> 255 VGPRs).
// Before touching this signature recheck gather_gemm_mfma_kernel<T, 64, 256, 1, false> with
// -Rpass-analysis=kernel-resource-usage against the previous build.
template <int SLAB_BYTES, int WAVES>
__device__ __forceinline__ void dma_weights(const char* src, char* dst, const int& wave, const int& lane) {
  static_assert(SLAB_BYTES % 1024 == 0, "weight slab must be a multiple of 1 KiB");
  constexpr int kUnits = SLAB_BYTES / 1024;  // one wave-instruction of LDS-DMA moves 1 KiB
#pragma unroll
  for (int it = 0; it < (kUnits + WAVES - 1) / WAVES; ++it) {
    const int u = it * WAVES + wave;  // wave-uniform 1-KiB unit
    if (u < kUnits) glds16(src + u * 1024 + lane * 16, __builtin_amdgcn_readfirstlane(lds_addr_of(dst + u * 1024)));
  }
}

// ---- epilogue: y = act((acc + bias) * scale + shift + residual), in fp32 before the rounding to the storage dtype ----
// results 4v .. 4v+3 of an accumulator
template <typename V>
__device__ __forceinline__ float4 acc4(const V& a, int v) {
  return make_float4(a[4 * v + 0], a[4 * v + 1], a[4 * v + 2], a[4 * v + 3]);
}
__device__ __forceinline__ float4 epi_bias(float4 o, float4 b) {
  return make_float4(o.x + b.x, o.y + b.y, o.z + b.z, o.w + b.w);
}
// per-channel affine (BatchNorm in inference mode)
__device__ __forceinline__ float4 epi_affine(float4 o, float4 s, float4 t) {
  return make_float4(o.x * s.x + t.x, o.y * s.y + t.y, o.z * s.z + t.z, o.w * s.w + t.w);
}
__device__ __forceinline__ float4 epi_relu(float4 o) {
  return make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
}
// rounded 16-B piece + residual piece (-> ReLU), rounded again
template <typename T, typename F>
__device__ __forceinline__ F add_residual(F o, F rv, int relu) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    float f = (float)o[q] + (float)rv[q];
    if (relu) f = fmaxf(f, 0.f);
    o[q] = (T)f;
  }
  return o;
}
// ---- host side -------------------------------------------------------------------------------------------------------
// The K <= 32 / K > 32 pair of a register-gather kernel (K0: one mask word, K1: MULTI; 256-thread kernels): raise the
// dynamic-LDS limit of both once per device, launch the one `multi` selects.
template <auto K0, auto K1, typename... Args>
inline int launch_multi(bool multi, dim3 grid, size_t lds_bytes, hipStream_t s, Args... args) {
  static unsigned long long attr_done = 0ull;  // per device (wcn_common.h)
  const int rc = once_per_device(attr_done, [lds_bytes] {
    bool ok = true;
    for (const void* f : {reinterpret_cast<const void*>(K0), reinterpret_cast<const void*>(K1)})
      ok = ok && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) == hipSuccess;
    return ok;
  });
  if (rc != WCN_SUCCESS) return rc;
  if (multi) hipLaunchKernelGGL(K1, grid, dim3(256), lds_bytes, s, args...);
  else hipLaunchKernelGGL(K0, grid, dim3(256), lds_bytes, s, args...);
  return launch_status();
}

// ---- which family takes a shape; the functions the gather-GEMM files and conv_api.hip share -----------------------------
// The layout of a packed weight image follows the family that consumes it, so the support query, the launcher and the
// weight packer all ask gather_gemm_family() - an image packed for one family and multiplied by another is garbage.
enum class GemmFamily { None, ChannelSplit, Mfma16, Mfma32 };
GemmFamily gather_gemm_family(int cin, int cout, int K, int dtype);                  // conv_mfma.hip

// per-family predicates (pure functions of the shape)
bool gather_gemm_cs_supported(int cin, int cout, int K, int dtype);                  // conv_mfma_cs.hip
bool mfma16_supported(int cin, int cout, int K, int dtype);                          // conv_mfma16.hip
bool mfma32_shape(int cin, int cout);                                                // conv_mfma.hip
bool mfma_gather_supported(int cin, int cout, int K, int dtype);                     // any family
bool mfma_grouped_supported(int cin, int cout, int K, int dtype);                    // per-group widths, 32x32x16 kernels
// what the packer has to know of the other two families' kernels
int cs_col_block(int cout);        // conv_mfma_cs.hip: width of the column blocks of the output
int mfma16_chunk(int cin, int cout);  // conv_mfma16.hip: reduction chunk per step
constexpr int kCsCIC = 64;         // channel-split family: input channels per step (one 128-B row piece)

// launchers: conv_gather_gemm_mfma (conv_mfma.hip) takes any supported shape and hands it to its family
int conv_gather_gemm_mfma(const void* in, const void* wp, void* out, const int32_t* nbr, const uint32_t* mask,
                          const int32_t* perm, const ConvEpilogue& epi, int64_t n_out, int cin, int cout, int K, int dtype,
                          float* out32, hipStream_t s);
int conv_gather_gemm_cs(const void* in, const void* wp, void* out, const int32_t* nbr, const uint32_t* mask,
                        const int32_t* perm, const ConvEpilogue& epi, int64_t n_out, int cin, int cout, int K, int dtype,
                        float* out32, hipStream_t s);
int conv_gather_gemm16(const void* in, const void* wp, void* out, const int32_t* nbr, const uint32_t* mask,
                       const int32_t* perm, const ConvEpilogue& epi, int64_t n_out, int cin, int cout, int K, int dtype,
                       float* out32, hipStream_t s);
int conv_gather_gemm_grouped(const void* in, const void* wp, void* out, const int32_t* nbr, const uint32_t* mask,
                             const int32_t* perm, const ConvEpilogue& epi, int64_t n_out, int cin, int cout, int groups,
                             int K, int dtype, hipStream_t s);

// weight packer (conv_mfma.hip); `w` fp32 (w_is_f32) or already in the 16-bit storage dtype
int pack_weight_mfma(const void* w, int w_is_f32, int K, int cin, int cout, int dtype, int transpose, int flip, void* packed,
                     hipStream_t s);
int pack_weight_grouped(const void* w, int w_is_f32, int K, int groups, int cin, int cout, int dtype, int transpose, int flip,
                        void* packed, hipStream_t s);
int pack_weight_cs_pair(const float* w, int K, int cin, int cout, int dtype, int flip_dgrad, void* packed_fwd,
                        void* packed_dgrad, hipStream_t s);

}  // namespace wcn
