// attn_varlen_d128.h - what the two kernel files of head size 128 share (attn_varlen_d128.hip: a wave pair per work item, and
// the entry points; attn_varlen_d128_shared.hip: P wave pairs per workgroup on staged tiles): the column split of a pair, the
// score-tile exchange, the grid cap, and the launchers of the shared-tile kernels.
#pragma once
#include "attn_varlen.h"

namespace wcn {

constexpr int kPairThreads = 128;                     // two waves
constexpr int kPairCols = 64;                         // columns of the head one wave owns
constexpr int kPairTr = kPairCols * kAttnPitch;       // elements of a wave's transposed image of its columns
constexpr int kPairTile = kAttnTile * kAttnTile;      // floats of an exchanged score tile
constexpr int64_t kAttnPairMaxGrid = 1 << 22;         // workgroups of one grid; the kernels stride beyond it

// A wave's partial score tile into its exchange slot: piece g of lane l at float 4 (64 g + l).
__device__ __forceinline__ void put_tile(float* __restrict__ slot, const a_f32x16& t, int lane) {
#pragma unroll
  for (int g = 0; g < 4; ++g)
    *reinterpret_cast<float4*>(slot + 4 * (64 * g + lane)) = make_float4(t[4 * g], t[4 * g + 1], t[4 * g + 2], t[4 * g + 3]);
}
// own + partner, element by element (the same bits in both waves).
__device__ __forceinline__ void add_tile(a_f32x16& t, const float* __restrict__ slot, int lane) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 x = *reinterpret_cast<const float4*>(slot + 4 * (64 * g + lane));
    t[4 * g] = t[4 * g] + x.x;
    t[4 * g + 1] = t[4 * g + 1] + x.y;
    t[4 * g + 2] = t[4 * g + 2] + x.z;
    t[4 * g + 3] = t[4 * g + 3] + x.w;
  }
}

static inline unsigned pair_grid(int64_t items) { return (unsigned)(items < kAttnPairMaxGrid ? items : kAttnPairMaxGrid); }

// The shared-tile kernels (attn_varlen_d128_shared.hip) on a checked call: the arguments of attn_pair_fwd_t / attn_pair_bwd_t
// with the dtype code, the same splits, partial layouts, combine / reduce / delta kernels.
int attn_wg_fwd(int dtype, const AttnCall& c, void* out, float* lse, const AttnKSplit& ks, hipStream_t s);
int attn_wg_bwd(int dtype, const AttnCall& c, const void* dout, const void* out, const float* lse, void* dq, int64_t dq_stride,
                void* dk, void* dv, int64_t dkv_stride, int q_splits, float* part, float* delta, const AttnKSplit& ks,
                hipStream_t s);

}  // namespace wcn
