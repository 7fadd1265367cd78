// ada_row.h - the row core of the row-streaming norm kernels (adaln.hip, ln_act.hip): a row of C channels is C / 8 pieces
// of 8 elements (one 16-B access of f16 / bf16, two of f32); G = the power of two >= min(C / 8, 64) lanes stand side by side
// on a row and hold it in registers, NCH = ceil(C / 8 / G) <= 4 pieces each; 64 / G rows share a wave; sums over a row
// cross its G lanes with an xor butterfly.  Stated here once, for every kernel of that shape:
//   the lane's place (row_lane), the group sum;
//   the forward's two-pass statistics (row_mean, row_dev, row_stats): the mean, then the sums of the deviations and of
//     their squares - the first corrects the mean's own rounding, which at |mean| >> sigma is what limits xhat;
//   the layout of stats (row_stats_st, row_stats_ld);
//   the backward's row step (row_xhat, row_mean_rcp, row_dx): dx = rstd (g - mean(g) - xhat mean(g xhat));
//   the host's geometry: lanes per row, pieces per lane, the two grids, the NCH dispatch.
// What differs between the kernels stays in them: what is loaded into the row, what g is, which column sums are kept.
#pragma once

#include "wcn_common.h"

namespace wcn {

constexpr int kAdaThreads = 256;
constexpr int kAdaChunk = 64;        // rows of one backward chunk
constexpr int kAdaMaxChannels = 2048;
constexpr int kAdaFwdBlocks = 4096;  // the forward's grid is capped here; its lane groups stride over the rows

// ---- device side ----------------------------------------------------------------------------------------------------------
// sum over the G = 1 << glog lanes of a group; every lane of the group receives the same bits
__device__ __forceinline__ float ada_group_sum(float v, int glog) {
  for (int m = 0; m < glog; ++m) v += __shfl_xor(v, 1 << m);
  return v;
}

// A lane's place in a launch of kAdaThreads-wide workgroups: lane gl of the G that stand on the row (or chunk) of lane
// group `unit`; it holds the pieces gl, gl + G, ... below nvec.
struct RowLane {
  int64_t unit;
  int gl, G, nvec;
};
__device__ __forceinline__ RowLane row_lane(int glog, int channels) {
  const int64_t v = (int64_t)blockIdx.x * kAdaThreads + threadIdx.x;
  RowLane l;
  l.unit = v >> glog;
  l.gl = (int)(v & ((1 << glog) - 1));
  l.G = 1 << glog;
  l.nvec = channels >> 3;
  return l;
}

// Forward statistics, two-pass.  With the row in f[NCH][8] (zeros where the lane has no piece or no row), s the lane's plain
// sum of it and fc = (float)C, a kernel runs
//   mean = row_mean(s, glog, fc);  sd = ss = 0;
//   for k, e:  row_dev(&f[k][e], act && gl + k * G < nvec, mean, sd, ss);      f now holds the deviations from `mean`
//   st = row_stats(mean, sd, ss, glog, fc, eps);                                xhat = (f - st.delta) * st.rstd
//   lane 0 of the group:  row_stats_st(stats, t, st);
// Every lane of a wave walks all of it: the butterflies need their partners.  The two loops stay in the kernels, and x is
// a pointer, on purpose: the compiler optimises an inlined function on its own first, and one that holds the unrolled
// loops over the row, or a load it may hoist out of the branch, comes out with up to 19 VGPRs more.
__device__ __forceinline__ float row_mean(float s, int glog, float fc) {
  return ada_group_sum(s, glog) / fc;  // a division: a constant row's mean is the constant, exactly
}
// one element: *x -> its deviation from the first mean (0 where masked), added to sd, its square to ss
__device__ __forceinline__ void row_dev(float* x, bool m, float mean, float& sd, float& ss) {
  const float d = m ? *x - mean : 0.f;
  *x = d;
  sd += d;
  ss += d * d;
}
struct RowStats {
  float mean, delta, rstd;
};
__device__ __forceinline__ RowStats row_stats(float mean, float sd, float ss, int glog, float fc, float eps) {
  const float delta = row_mean(sd, glog, fc);  // what the rounded mean missed
  ss = row_mean(ss, glog, fc);
  const float var = fmaxf(ss - delta * delta, 0.f);
  const float rstd = 1.0f / sqrtf(var + eps);
  mean += delta;
  return {mean, delta, rstd};
}

// stats [rows, 2] = (mean, rstd), 8-B aligned
__device__ __forceinline__ void row_stats_st(float* __restrict__ stats, int64_t t, const RowStats& st) {
  *reinterpret_cast<float2*>(stats + 2 * t) = make_float2(st.mean, st.rstd);
}
__device__ __forceinline__ void row_stats_ld(const float* __restrict__ stats, int64_t t, float& mean, float& rstd) {
  const float2 st = *reinterpret_cast<const float2*>(stats + 2 * t);
  mean = st.x;
  rstd = st.y;
}

// Backward row step: with g the gradient arriving at xhat, s1 and s2 the row means of g and of g xhat (the lane's sums
// through row_mean_rcp, inv_c = 1 / (float)C), dx = rstd (g - s1 - xhat s2).
__device__ __forceinline__ float row_xhat(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float row_mean_rcp(float s, int glog, float inv_c) { return ada_group_sum(s, glog) * inv_c; }
__device__ __forceinline__ float row_dx(float rstd, float gd, float xh, float s1, float s2) {
  return rstd * (gd - s1 - xh * s2);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// lanes per row: G = 1 << row_glog(pieces of a row)
inline int row_glog(int pieces) {
  int glog = 0;
  while ((1 << glog) < pieces && glog < 6) ++glog;
  return glog;
}

// the forward's grid: a lane group per row up to the cap, striding over the rows beyond; returns the blocks, sets *units
inline unsigned row_fwd_grid(int64_t rows, int glog, int64_t* units) {
  const int64_t per_block = kAdaThreads >> glog;
  int64_t blocks = ceil_div(rows, per_block);
  if (blocks > kAdaFwdBlocks) blocks = kAdaFwdBlocks;
  *units = blocks * per_block;
  return (unsigned)blocks;
}
// the backward's grid: a lane group per chunk of kAdaChunk rows
inline unsigned row_bwd_grid(int64_t rows, int glog, int64_t* units) {
  *units = ceil_div(rows, kAdaChunk);
  return (unsigned)ceil_div(*units, kAdaThreads >> glog);
}

// f(std::integral_constant<int, NCH>) for NCH = the pieces a lane holds
template <typename F>
inline void row_with_nch(int channels, int glog, F&& f) {
  switch ((int)ceil_div(channels / 8, 1 << glog)) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

}  // namespace wcn
