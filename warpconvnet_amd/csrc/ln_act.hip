// ln_act.hip - the per-voxel glue of the sparse U-Net residual blocks (reference: nn/modules/sparse_unet.py runs, between
// two convolutions, x.float() -> layer_norm -> .to(dtype) -> silu as five or six [N, C] passes, and closes with
// h + repeat_interleave(x) or h + reshape(...).mean(-1)).  One row-streaming pass per site and direction:
//   LN (+ affine) (+ SiLU)   y = act(LN(x) * weight + bias), biased variance, fp32, rounded once; launch shape, two-pass
//                            statistics and backward row step are ada_row.h's (G lanes hold a row in registers, <= 4
//                            pieces each), as in adaln.hip; here are the affine pair, SiLU and their column sums.
//     forward   the lane groups stride over the rows; writes stats [rows, 2] = (mean, rstd).
//     backward  z = xhat * weight + bias is formed again in fp32 from x and stats, never read back from the rounded y.
//               Lane group u owns the kAdaChunk rows of chunk u, keeps the column sums of dweight / dbias in registers and
//               writes them once to the partial slot u; ln_act_final_kernel adds the slots in a fixed order.  No float
//               atomics, no zero-filled workspace: two runs are bit-identical.
//   spread   out[n, c * r + j] = alpha * x[n, c] (+ h[n, c * r + j])        the decoder's skip, and the fold's gradient
//   fold     out[n, c] = alpha * sum_{j < g} x[n, c * g + j] (+ h[n, c])    the encoder's skip, and the spread's gradient
//     One lane per 8-element piece of an output row, 16-B accesses, where the narrow side's channel count is a multiple of
//     8 and r / g is 1, 2, 4 or 8 (what halving / doubling widths around a factor-2 resample give; every index into the
//     lane's registers is then a compile-time constant, so nothing goes to scratch); one lane per output element otherwise.
//   permuted rows   the attention sub-layer of a serialized-attention block, x + drop_path(attn(norm1(x)[perm])[inverse]), around
//                   the attention itself: two row passes instead of LayerNorm, two gathers, a mask multiply and an add.
//     LN + permute  y[i] = LN(x[index[i]]) * weight + bias: the LN forward above with the row read through `index`; stats are
//                   kept per SOURCE row j = index[i].  The backward is a gather too: lane group u owns the source rows of chunk
//                   u, reads dy at i = inverse[j], and writes dx[j] once; dweight / dbias go through the same partial slots
//                   and ln_act_final_kernel.  No float atomics, no zero-filled workspace.
//     permute + add out[t] = residual[t] + scale * y[index[t]]; `scale` the fp32 per-row stochastic-depth factor, read at t
//                   (forward) or at index[t] (the backward, which is the same kernel with the inverse index and no residual).
//     Index guard: an index is an int64 read from memory and compared as unsigned with `rows` before any address is formed
//     from it ((uint64_t)j < (uint64_t)rows: negative values fail too).  A row whose index fails is written as zeros (in the
//     LN backward: dx[j] = 0 and nothing is added to the column sums); no load or store ever uses the failed value.
#include <limits.h>

#include <cmath>

#include "ada_row.h"

namespace wcn {

struct LnGeom {
  int64_t rows;
  int64_t units;  // lane groups of the launch: the forward's stride over the rows, the backward's chunks
  int channels, glog;
  float eps;
};

// hardware exp2 and reciprocal (1 ulp each): z -> -inf gives 1 / inf = 0, never a NaN
__device__ __forceinline__ float ln_sigmoid(float z) { return __builtin_amdgcn_rcpf(1.0f + __expf(-z)); }

template <typename T, int NCH, bool AFFINE, bool SILU>
__global__ __launch_bounds__(kAdaThreads) void ln_act_fwd_kernel(const T* __restrict__ x, const float* __restrict__ weight,
                                                                 const float* __restrict__ bias, T* __restrict__ y,
                                                                 float* __restrict__ stats, const LnGeom g) {
  const RowLane l = row_lane(g.glog, g.channels);
  const int C = g.channels;
  const float fc = (float)C;

  // every lane of a wave walks the same number of trips: the butterfly needs its partners
  for (int64_t t0 = 0; t0 < g.rows; t0 += g.units) {
    const int64_t t = t0 + l.unit;
    const bool act = t < g.rows;
    float f[NCH][8];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * l.G;
      if (act && c < l.nvec) {
        ld_vec(x + t * C + c * 8, f[k]);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += f[k][e];
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[k][e] = 0.f;
      }
    }
    const float mean = row_mean(s, g.glog, fc);
    float sd = 0.f, ss = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const bool m = act && l.gl + k * l.G < l.nvec;
#pragma unroll
      for (int e = 0; e < 8; ++e) row_dev(&f[k][e], m, mean, sd, ss);
    }
    const RowStats st = row_stats(mean, sd, ss, g.glog, fc, g.eps);
    if (act && l.gl == 0) row_stats_st(stats, t, st);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * l.G;
      if (act && c < l.nvec) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (f[k][e] - st.delta) * st.rstd;
        if constexpr (AFFINE) {
          float w[8], b[8];
          ld_vec(weight + c * 8, w);
          ld_vec(bias + c * 8, b);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = o[e] * w[e] + b[e];
        }
        if constexpr (SILU) {
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] *= ln_sigmoid(o[e]);
        }
        st_vec(y + t * C + c * 8, o);
      }
    }
  }
}

// partial [units][2][C]: 0 = dweight, 1 = dbias
template <typename T, int NCH, bool AFFINE, bool SILU>
__global__ __launch_bounds__(kAdaThreads) void ln_act_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                 const float* __restrict__ weight,
                                                                 const float* __restrict__ bias,
                                                                 const float* __restrict__ stats, T* __restrict__ dx,
                                                                 float* __restrict__ partial, const LnGeom g) {
  const RowLane l = row_lane(g.glog, g.channels);
  const int C = g.channels;
  const float inv_c = 1.0f / (float)C;
  const bool live = l.unit < g.units;

  float a_w[AFFINE ? NCH : 1][8], a_b[AFFINE ? NCH : 1][8];
  if constexpr (AFFINE) {
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) { a_w[k][e] = 0.f; a_b[k][e] = 0.f; }
  }

#pragma unroll 1
  for (int i = 0; i < kAdaChunk; ++i) {
    const int64_t t = l.unit * kAdaChunk + i;
    const bool act = live && t < g.rows;
    float gd[NCH][8], xh[NCH][8];  // g * weight; xhat
    float mean = 0.f, rstd = 0.f, s1 = 0.f, s2 = 0.f;
    if (act) row_stats_ld(stats, t, mean, rstd);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * l.G;
      if (act && c < l.nvec) {
        const int64_t at = t * C + c * 8;
        float xv[8], w[8], b[8];
        ld_vec(dy + at, gd[k]);
        ld_vec(x + at, xv);
        if constexpr (AFFINE) {
          ld_vec(weight + c * 8, w);
          ld_vec(bias + c * 8, b);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float d = gd[k][e];
          xh[k][e] = row_xhat(xv[e], mean, rstd);
          if constexpr (SILU) {
            float z = xh[k][e];
            if constexpr (AFFINE) z = z * w[e] + b[e];
            const float sg = ln_sigmoid(z);
            d *= sg * (1.0f + z * (1.0f - sg));
          }
          if constexpr (AFFINE) {
            a_b[k][e] += d;
            a_w[k][e] += d * xh[k][e];
            d *= w[e];
          }
          gd[k][e] = d;
          s1 += d;
          s2 += d * xh[k][e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { gd[k][e] = 0.f; xh[k][e] = 0.f; }
      }
    }
    s1 = row_mean_rcp(s1, g.glog, inv_c);
    s2 = row_mean_rcp(s2, g.glog, inv_c);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * l.G;
      if (act && c < l.nvec) {
        float r[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = row_dx(rstd, gd[k][e], xh[k][e], s1, s2);
        st_vec(dx + t * C + c * 8, r);
      }
    }
  }
  if constexpr (AFFINE) {
    if (live) {  // every chunk has a row, and every column of its slot a lane
      float* p = partial + l.unit * 2 * (int64_t)C;
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        const int c = l.gl + k * l.G;
        if (c < l.nvec) {
          st_vec(p + c * 8, a_w[k]);
          st_vec(p + C + c * 8, a_b[k]);
        }
      }
    }
  }
}

// ---- LN + permute ---------------------------------------------------------------------------------------------------------
// y[t] = LN(x[index[t]]) (* weight + bias); stats[index[t]] = (mean, rstd).  The row loop of ln_act_fwd_kernel; `act` is the
// index guard as well: a lane group whose row has no valid source walks the butterflies on zeros and writes a zero row.
template <typename T, int NCH, bool AFFINE>
__global__ __launch_bounds__(kAdaThreads) void ln_permute_fwd_kernel(const T* __restrict__ x, const int64_t* __restrict__ index,
                                                                     const float* __restrict__ weight,
                                                                     const float* __restrict__ bias, T* __restrict__ y,
                                                                     float* __restrict__ stats, const LnGeom g) {
  const RowLane l = row_lane(g.glog, g.channels);
  const int C = g.channels;
  const float fc = (float)C;

  for (int64_t t0 = 0; t0 < g.rows; t0 += g.units) {
    const int64_t t = t0 + l.unit;
    const bool live = t < g.rows;
    const int64_t j = live ? index[t] : -1;  // the same in every lane of the group
    const bool act = (uint64_t)j < (uint64_t)g.rows;
    float f[NCH][8];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * l.G;
      if (act && c < l.nvec) {
        ld_vec(x + j * C + c * 8, f[k]);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += f[k][e];
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[k][e] = 0.f;
      }
    }
    const float mean = row_mean(s, g.glog, fc);
    float sd = 0.f, ss = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const bool m = act && l.gl + k * l.G < l.nvec;
#pragma unroll
      for (int e = 0; e < 8; ++e) row_dev(&f[k][e], m, mean, sd, ss);
    }
    const RowStats st = row_stats(mean, sd, ss, g.glog, fc, g.eps);
    if (act && l.gl == 0) row_stats_st(stats, j, st);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * l.G;
      if (live && c < l.nvec) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (f[k][e] - st.delta) * st.rstd;
        if constexpr (AFFINE) {
          float w[8], b[8];
          ld_vec(weight + c * 8, w);
          ld_vec(bias + c * 8, b);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = o[e] * w[e] + b[e];
        }
        if (!act) {
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = 0.f;
        }
        st_vec(y + t * C + c * 8, o);
      }
    }
  }
}

// Lane group u owns the source rows j of chunk u: dy is read at i = inverse[j], x and stats at j, dx[j] written once.
// partial [units][2][C] as in ln_act_bwd_kernel.
template <typename T, int NCH, bool AFFINE>
__global__ __launch_bounds__(kAdaThreads) void ln_permute_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                     const int64_t* __restrict__ inverse,
                                                                     const float* __restrict__ weight,
                                                                     const float* __restrict__ stats, T* __restrict__ dx,
                                                                     float* __restrict__ partial, const LnGeom g) {
  const RowLane l = row_lane(g.glog, g.channels);
  const int C = g.channels;
  const float inv_c = 1.0f / (float)C;
  const bool live = l.unit < g.units;

  float a_w[AFFINE ? NCH : 1][8], a_b[AFFINE ? NCH : 1][8];
  if constexpr (AFFINE) {
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) { a_w[k][e] = 0.f; a_b[k][e] = 0.f; }
  }

#pragma unroll 1
  for (int r = 0; r < kAdaChunk; ++r) {
    const int64_t j = l.unit * kAdaChunk + r;
    const bool row = live && j < g.rows;
    const int64_t i = row ? inverse[j] : -1;
    const bool act = (uint64_t)i < (uint64_t)g.rows;
    float gd[NCH][8], xh[NCH][8];  // g * weight; xhat
    float mean = 0.f, rstd = 0.f, s1 = 0.f, s2 = 0.f;
    if (act) row_stats_ld(stats, j, mean, rstd);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * l.G;
      if (act && c < l.nvec) {
        float xv[8], w[8];
        ld_vec(dy + i * C + c * 8, gd[k]);
        ld_vec(x + j * C + c * 8, xv);
        if constexpr (AFFINE) ld_vec(weight + c * 8, w);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float d = gd[k][e];
          xh[k][e] = row_xhat(xv[e], mean, rstd);
          if constexpr (AFFINE) {
            a_b[k][e] += d;
            a_w[k][e] += d * xh[k][e];
            d *= w[e];
          }
          gd[k][e] = d;
          s1 += d;
          s2 += d * xh[k][e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { gd[k][e] = 0.f; xh[k][e] = 0.f; }
      }
    }
    s1 = row_mean_rcp(s1, g.glog, inv_c);
    s2 = row_mean_rcp(s2, g.glog, inv_c);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * l.G;
      if (row && c < l.nvec) {  // without a valid i: gd = xh = 0 and rstd = 0, a row of zeros
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = row_dx(rstd, gd[k][e], xh[k][e], s1, s2);
        st_vec(dx + j * C + c * 8, o);
      }
    }
  }
  if constexpr (AFFINE) {
    if (live) {
      float* p = partial + l.unit * 2 * (int64_t)C;
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        const int c = l.gl + k * l.G;
        if (c < l.nvec) {
          st_vec(p + c * 8, a_w[k]);
          st_vec(p + C + c * 8, a_b[k]);
        }
      }
    }
  }
}

// ---- permute + add --------------------------------------------------------------------------------------------------------
// out[t] = residual[t] + scale * y[index[t]]: one lane per 8-element piece, G lanes side by side on a row.  `residual` may be
// NULL; SCALED = false is one fp32 add per element.  scale is read at t, or at index[t] with scale_at_source.
struct PermGeom {
  int64_t rows;
  int64_t units;
  int channels, glog;
  int scale_at_source;
};

template <typename T, bool SCALED>
__global__ __launch_bounds__(kAdaThreads) void permute_add_kernel(const T* __restrict__ y, const int64_t* __restrict__ index,
                                                                  const T* __restrict__ residual,
                                                                  const float* __restrict__ scale, T* __restrict__ out,
                                                                  const PermGeom g) {
  const RowLane l = row_lane(g.glog, g.channels);
  const int C = g.channels;
  for (int64_t t = l.unit; t < g.rows; t += g.units) {
    const int64_t i = index[t];
    const bool ok = (uint64_t)i < (uint64_t)g.rows;
    float sc = 1.f;
    if constexpr (SCALED) sc = ok ? scale[g.scale_at_source ? i : t] : 0.f;
    for (int p = l.gl; p < l.nvec; p += l.G) {
      float o[8];
      if (ok) {
        ld_vec(y + i * C + p * 8, o);
        if constexpr (SCALED) {
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] *= sc;
        }
        if (residual != nullptr) {  // the same in every lane
          float rv[8];
          ld_vec(residual + t * C + p * 8, rv);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = rv[e] + o[e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = 0.f;
      }
      st_vec(out + t * C + p * 8, o);
    }
  }
}

// second level of the column sums: 32 columns x 32 slot slices per workgroup, one of the two sums each; both levels in a
// fixed order
constexpr int kLnFinalSlices = 32;

__global__ __launch_bounds__(32 * kLnFinalSlices) void ln_act_final_kernel(const float* __restrict__ partial, int64_t slots,
                                                                           int C, float* __restrict__ dweight,
                                                                           float* __restrict__ dbias) {
  __shared__ float s[kLnFinalSlices][33];
  const int which = blockIdx.y;
  float* out = which == 0 ? dweight : dbias;
  const int cl = threadIdx.x & 31, q = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + cl;
  float sum = 0.f;
  if (col < C)
    for (int64_t sl = q; sl < slots; sl += kLnFinalSlices) sum += partial[(sl * 2 + which) * C + col];
  s[q][cl] = sum;
  __syncthreads();
  if (q == 0 && col < C) {
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < kLnFinalSlices; ++i) tot += s[i][cl];
    out[col] = tot;
  }
}

// ---- channel spread / fold -------------------------------------------------------------------------------------------------
struct SkipGeom {
  int64_t rows;
  int64_t units;  // lane groups of the launch: the stride over the rows
  int cout;       // channels of an output row
  int ratio;      // r or g (the element kernels; the piece kernels have it as R)
  int glog;
  float alpha;
};

template <typename T> __device__ __forceinline__ float skip_ld(const T* p) { return (float)*p; }

// One lane per 8-element piece of an output row; G = 1 << glog lanes side by side on a row, striding over its pieces.
// FOLD = false: the piece [8p, 8p + 8) of out reads the 8 / R elements of x from 8p / R on.
// FOLD = true:  it reads the R pieces of x from piece p * R on; output e is the sum of the R elements from e * R on.
template <typename T, int R, bool FOLD>
__global__ __launch_bounds__(kAdaThreads) void channel_pieces_kernel(const T* __restrict__ x, const T* __restrict__ h,
                                                                     T* __restrict__ out, const SkipGeom g) {
  const RowLane l = row_lane(g.glog, g.cout);
  const int64_t cx = FOLD ? (int64_t)g.cout * R : g.cout / R;  // channels of a row of x
  for (int64_t t = l.unit; t < g.rows; t += g.units) {
    for (int p = l.gl; p < l.nvec; p += l.G) {
      float o[8];
      if constexpr (FOLD) {
        float f[R][8];
#pragma unroll
        for (int k = 0; k < R; ++k) ld_vec(x + t * cx + ((int64_t)p * R + k) * 8, f[k]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float s = 0.f;
#pragma unroll
          for (int j = 0; j < R; ++j) s += f[(e * R + j) >> 3][(e * R + j) & 7];
          o[e] = g.alpha * s;
        }
      } else if constexpr (R == 1) {
        ld_vec(x + t * cx + p * 8, o);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] *= g.alpha;
      } else {
        float f[8 / R];
        const T* src = x + t * cx + p * (8 / R);
#pragma unroll
        for (int k = 0; k < 8 / R; ++k) f[k] = g.alpha * skip_ld(src + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = f[e / R];
      }
      const int64_t at = t * g.cout + p * 8;
      if (h != nullptr) {  // the same in every lane
        float hv[8];
        ld_vec(h + at, hv);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += hv[e];
      }
      st_vec(out + at, o);
    }
  }
}

// One lane per output element: any channel count, any ratio, any alignment.
template <typename T, bool FOLD>
__global__ __launch_bounds__(kAdaThreads) void channel_elements_kernel(const T* __restrict__ x, const T* __restrict__ h,
                                                                       T* __restrict__ out, const SkipGeom g) {
  const int64_t total = g.rows * g.cout;
  const int64_t stride = (int64_t)gridDim.x * kAdaThreads;
  for (int64_t i = (int64_t)blockIdx.x * kAdaThreads + threadIdx.x; i < total; i += stride) {
    const int64_t t = i / g.cout;
    const int c = (int)(i - t * g.cout);
    float o;
    if constexpr (FOLD) {
      const T* src = x + (t * g.cout + c) * g.ratio;  // a row of x has cout * g channels
      float s = 0.f;
      for (int j = 0; j < g.ratio; ++j) s += skip_ld(src + j);
      o = g.alpha * s;
    } else {
      o = g.alpha * skip_ld(x + t * (g.cout / g.ratio) + c / g.ratio);
    }
    if (h != nullptr) o += skip_ld(h + i);
    out[i] = (T)o;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
static LnGeom ln_geom(int64_t rows, int channels, float eps) {
  LnGeom g;
  g.rows = rows;
  g.units = 0;
  g.channels = channels;
  g.glog = row_glog(channels / 8);
  g.eps = eps;
  return g;
}

// Shared argument checks.  Returns WCN_SUCCESS, an error, or 1 = valid but nothing to launch.
static int ln_check(int64_t rows, int32_t channels, int32_t dtype, int32_t act, const float* weight, const float* bias) {
  if (rows < 0) return WCN_ERROR_INVALID_PARAMETERS;
  if (!wcn_ln_act_supported(channels, dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (rows > INT32_MAX || (act != 0 && act != 1)) return WCN_ERROR_INVALID_PARAMETERS;
  if ((weight != nullptr) != (bias != nullptr)) return WCN_ERROR_INVALID_PARAMETERS;
  return rows == 0 ? 1 : WCN_SUCCESS;
}

template <typename T, bool AFFINE, bool SILU>
static int ln_fwd_t(const void* x, const float* weight, const float* bias, void* y, float* stats, LnGeom g, hipStream_t s) {
  const unsigned blocks = row_fwd_grid(g.rows, g.glog, &g.units);
  row_with_nch(g.channels, g.glog, [&](auto nch) {
    hipLaunchKernelGGL((ln_act_fwd_kernel<T, nch(), AFFINE, SILU>), dim3(blocks), dim3(kAdaThreads), 0, s, (const T*)x,
                       weight, bias, (T*)y, stats, g);
  });
  return launch_status();
}

template <typename T, bool AFFINE, bool SILU>
static int ln_bwd_t(const void* dy, const void* x, const float* weight, const float* bias, const float* stats, void* dx,
                    float* partial, LnGeom g, hipStream_t s) {
  const unsigned blocks = row_bwd_grid(g.rows, g.glog, &g.units);
  row_with_nch(g.channels, g.glog, [&](auto nch) {
    hipLaunchKernelGGL((ln_act_bwd_kernel<T, nch(), AFFINE, SILU>), dim3(blocks), dim3(kAdaThreads), 0, s, (const T*)dy,
                       (const T*)x, weight, bias, stats, (T*)dx, partial, g);
  });
  return launch_status();
}

template <typename T, bool AFFINE>
static int ln_perm_fwd_t(const void* x, const int64_t* index, const float* weight, const float* bias, void* y, float* stats,
                         LnGeom g, hipStream_t s) {
  const unsigned blocks = row_fwd_grid(g.rows, g.glog, &g.units);
  row_with_nch(g.channels, g.glog, [&](auto nch) {
    hipLaunchKernelGGL((ln_permute_fwd_kernel<T, nch(), AFFINE>), dim3(blocks), dim3(kAdaThreads), 0, s, (const T*)x, index,
                       weight, bias, (T*)y, stats, g);
  });
  return launch_status();
}

template <typename T, bool AFFINE>
static int ln_perm_bwd_t(const void* dy, const void* x, const int64_t* inverse, const float* weight, const float* stats,
                         void* dx, float* partial, LnGeom g, hipStream_t s) {
  const unsigned blocks = row_bwd_grid(g.rows, g.glog, &g.units);
  row_with_nch(g.channels, g.glog, [&](auto nch) {
    hipLaunchKernelGGL((ln_permute_bwd_kernel<T, nch(), AFFINE>), dim3(blocks), dim3(kAdaThreads), 0, s, (const T*)dy,
                       (const T*)x, inverse, weight, stats, (T*)dx, partial, g);
  });
  return launch_status();
}

template <typename T>
static int permute_add_t(const void* y, const int64_t* index, const void* residual, const float* scale, void* out, PermGeom g,
                         hipStream_t s) {
  const unsigned blocks = row_fwd_grid(g.rows, g.glog, &g.units);
  if (scale != nullptr)
    hipLaunchKernelGGL((permute_add_kernel<T, true>), dim3(blocks), dim3(kAdaThreads), 0, s, (const T*)y, index,
                       (const T*)residual, scale, (T*)out, g);
  else
    hipLaunchKernelGGL((permute_add_kernel<T, false>), dim3(blocks), dim3(kAdaThreads), 0, s, (const T*)y, index,
                       (const T*)residual, scale, (T*)out, g);
  return launch_status();
}

// the four uses of one dtype
#define WCN_LN_USES(FN, T, ...)                                                                \
  (affine ? (act ? FN<T, true, true>(__VA_ARGS__) : FN<T, true, false>(__VA_ARGS__))           \
          : (act ? FN<T, false, true>(__VA_ARGS__) : FN<T, false, false>(__VA_ARGS__)))
#define WCN_LN_DTYPES(FN, ...) \
  with_dtype(dtype, [&](auto el) { return WCN_LN_USES(FN, decltype(el), __VA_ARGS__); })

template <typename T, bool FOLD>
static int skip_t(const void* x, const void* h, void* out, SkipGeom g, bool pieces, hipStream_t s) {
  const T *xp = (const T*)x, *hp = (const T*)h;
  T* op = (T*)out;
  if (!pieces) {
    int64_t blocks = ceil_div(g.rows * g.cout, kAdaThreads);
    if (blocks > kAdaFwdBlocks) blocks = kAdaFwdBlocks;
    hipLaunchKernelGGL((channel_elements_kernel<T, FOLD>), dim3((unsigned)blocks), dim3(kAdaThreads), 0, s, xp, hp, op, g);
    return launch_status();
  }
  g.glog = row_glog(g.cout / 8);
  const unsigned blocks = row_fwd_grid(g.rows, g.glog, &g.units);
#define WCN_SKIP(R) \
  hipLaunchKernelGGL((channel_pieces_kernel<T, R, FOLD>), dim3(blocks), dim3(kAdaThreads), 0, s, xp, hp, op, g)
  switch (g.ratio) {
    case 1: WCN_SKIP(1); break;
    case 2: WCN_SKIP(2); break;
    case 4: WCN_SKIP(4); break;
    default: WCN_SKIP(8); break;
  }
#undef WCN_SKIP
  return launch_status();
}

// narrow = the channel count of the narrow side (x of a spread, out of a fold); the output row has `cout` channels
static int skip_run(bool fold, const void* x, const void* h, int64_t rows, int64_t narrow, int64_t ratio, float alpha,
                    int32_t dtype, void* out, hipStream_t s) {
  if (rows < 0 || narrow < 1 || ratio < 1) return WCN_ERROR_INVALID_PARAMETERS;
  if (!dtype_ok(dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (narrow * ratio > INT32_MAX) return WCN_ERROR_UNSUPPORTED_CONFIG;  // a row's channels are counted in int32
  if (rows > INT32_MAX || !std::isfinite(alpha)) return WCN_ERROR_INVALID_PARAMETERS;
  if (rows == 0) return WCN_SUCCESS;
  if (!x || !out) return WCN_ERROR_INVALID_PARAMETERS;
  const size_t el = dtype == WCN_F32 ? 4 : 2;
  if (!aligned_to(x, el) || !aligned_to(h, el) || !aligned_to(out, el)) return WCN_ERROR_INVALID_PARAMETERS;
  SkipGeom g;
  g.rows = rows;
  g.units = 0;
  g.cout = (int)(fold ? narrow : narrow * ratio);
  g.ratio = (int)ratio;
  g.glog = 0;
  g.alpha = alpha;
  // 16-B pieces: every row of both sides starts on the 16-B grid, and a piece's indices are compile-time constants
  const bool pieces = narrow % 8 == 0 && (ratio == 1 || ratio == 2 || ratio == 4 || ratio == 8) && aligned_to(x, 16) &&
                      aligned_to(h, 16) && aligned_to(out, 16);
  return with_dtype(dtype, [&](auto el) {
    using T = decltype(el);
    return fold ? skip_t<T, true>(x, h, out, g, pieces, s) : skip_t<T, false>(x, h, out, g, pieces, s);
  });
}

}  // namespace wcn

using namespace wcn;

int wcn_ln_act_supported(int32_t channels, int32_t dtype) { return wcn_adaln_supported(channels, dtype); }

size_t wcn_ln_act_workspace_bytes(int64_t rows, int32_t channels) {
  if (rows <= 0 || channels < 1) return 0;
  return (size_t)ceil_div(rows, kAdaChunk) * 2 * (size_t)channels * sizeof(float);
}

int wcn_ln_act_fwd(const void* x, const float* weight, const float* bias, int64_t rows, int32_t channels, float eps,
                   int32_t act, int32_t dtype, void* y, float* stats, wcn_stream_t stream) {
  int st = ln_check(rows, channels, dtype, act, weight, bias);
  if ((st == WCN_SUCCESS || st == 1) && !(eps >= 0.f && std::isfinite(eps))) st = WCN_ERROR_INVALID_PARAMETERS;
  if (st == WCN_SUCCESS) {
    if (!x || !y || !stats) st = WCN_ERROR_INVALID_PARAMETERS;
    else if (!aligned_to(x, 16) || !aligned_to(weight, 16) || !aligned_to(bias, 16) || !aligned_to(y, 16) ||
             !aligned_to(stats, 8))
      st = WCN_ERROR_INVALID_PARAMETERS;
  }
  if (st != WCN_SUCCESS) return st == 1 ? WCN_SUCCESS : st;
  const bool affine = weight != nullptr;
  const LnGeom g = ln_geom(rows, channels, eps);
  return WCN_LN_DTYPES(ln_fwd_t, x, weight, bias, y, stats, g, (hipStream_t)stream);
}

int wcn_ln_act_bwd(const void* dy, const void* x, const float* weight, const float* bias, const float* stats, int64_t rows,
                   int32_t channels, int32_t act, int32_t dtype, void* dx, float* dweight, float* dbias, void* workspace,
                   size_t workspace_bytes, wcn_stream_t stream) {
  const bool affine = weight != nullptr;
  int st = ln_check(rows, channels, dtype, act, weight, bias);
  if ((st == WCN_SUCCESS || st == 1) && affine && workspace_bytes < wcn_ln_act_workspace_bytes(rows, channels))
    st = WCN_ERROR_INVALID_PARAMETERS;
  if (st == WCN_SUCCESS) {
    if (!dy || !x || !stats || !dx || (affine && (!dweight || !dbias || !workspace))) st = WCN_ERROR_INVALID_PARAMETERS;
    else if (!aligned_to(dy, 16) || !aligned_to(x, 16) || !aligned_to(weight, 16) || !aligned_to(bias, 16) ||
             !aligned_to(stats, 8) || !aligned_to(dx, 16) || !aligned_to(dweight, 4) || !aligned_to(dbias, 4) ||
             (affine && !aligned_to(workspace, 16)))
      st = WCN_ERROR_INVALID_PARAMETERS;
  }
  if (st != WCN_SUCCESS) return st == 1 ? WCN_SUCCESS : st;
  hipStream_t s = (hipStream_t)stream;
  const LnGeom g = ln_geom(rows, channels, 0.f);
  float* partial = affine ? (float*)workspace : nullptr;
  st = WCN_LN_DTYPES(ln_bwd_t, dy, x, weight, bias, stats, dx, partial, g, s);
  if (st != WCN_SUCCESS || !affine) return st;
  hipLaunchKernelGGL(ln_act_final_kernel, dim3((unsigned)ceil_div(channels, 32), 2), dim3(32 * kLnFinalSlices), 0, s,
                     (const float*)partial, ceil_div(rows, kAdaChunk), channels, dweight, dbias);
  return launch_status();
}

int wcn_ln_permute_fwd(const void* x, const int64_t* index, const float* weight, const float* bias, int64_t rows,
                       int32_t channels, float eps, int32_t dtype, void* y, float* stats, wcn_stream_t stream) {
  int st = ln_check(rows, channels, dtype, 0, weight, bias);
  if ((st == WCN_SUCCESS || st == 1) && !(eps >= 0.f && std::isfinite(eps))) st = WCN_ERROR_INVALID_PARAMETERS;
  if (st == WCN_SUCCESS) {
    if (!x || !index || !y || !stats) st = WCN_ERROR_INVALID_PARAMETERS;
    else if (!aligned_to(x, 16) || !aligned_to(index, 8) || !aligned_to(weight, 16) || !aligned_to(bias, 16) ||
             !aligned_to(y, 16) || !aligned_to(stats, 8))
      st = WCN_ERROR_INVALID_PARAMETERS;
  }
  if (st != WCN_SUCCESS) return st == 1 ? WCN_SUCCESS : st;
  const LnGeom g = ln_geom(rows, channels, eps);
  return with_dtype(dtype, [&](auto el) {
    using T = decltype(el);
    return weight != nullptr ? ln_perm_fwd_t<T, true>(x, index, weight, bias, y, stats, g, (hipStream_t)stream)
                             : ln_perm_fwd_t<T, false>(x, index, weight, bias, y, stats, g, (hipStream_t)stream);
  });
}

int wcn_ln_permute_bwd(const void* dy, const void* x, const int64_t* inverse, const float* weight, const float* stats,
                       int64_t rows, int32_t channels, int32_t dtype, void* dx, float* dweight, float* dbias, void* workspace,
                       size_t workspace_bytes, wcn_stream_t stream) {
  const bool affine = weight != nullptr;
  int st = ln_check(rows, channels, dtype, 0, weight, weight);
  if ((st == WCN_SUCCESS || st == 1) && affine && workspace_bytes < wcn_ln_act_workspace_bytes(rows, channels))
    st = WCN_ERROR_INVALID_PARAMETERS;
  if (st == WCN_SUCCESS) {
    if (!dy || !x || !inverse || !stats || !dx || (affine && (!dweight || !dbias || !workspace)))
      st = WCN_ERROR_INVALID_PARAMETERS;
    else if (!aligned_to(dy, 16) || !aligned_to(x, 16) || !aligned_to(inverse, 8) || !aligned_to(weight, 16) ||
             !aligned_to(stats, 8) || !aligned_to(dx, 16) || !aligned_to(dweight, 4) || !aligned_to(dbias, 4) ||
             (affine && !aligned_to(workspace, 16)))
      st = WCN_ERROR_INVALID_PARAMETERS;
  }
  if (st != WCN_SUCCESS) return st == 1 ? WCN_SUCCESS : st;
  hipStream_t s = (hipStream_t)stream;
  const LnGeom g = ln_geom(rows, channels, 0.f);
  float* partial = affine ? (float*)workspace : nullptr;
  st = with_dtype(dtype, [&](auto el) {
    using T = decltype(el);
    return affine ? ln_perm_bwd_t<T, true>(dy, x, inverse, weight, stats, dx, partial, g, s)
                  : ln_perm_bwd_t<T, false>(dy, x, inverse, weight, stats, dx, partial, g, s);
  });
  if (st != WCN_SUCCESS || !affine) return st;
  hipLaunchKernelGGL(ln_act_final_kernel, dim3((unsigned)ceil_div(channels, 32), 2), dim3(32 * kLnFinalSlices), 0, s,
                     (const float*)partial, ceil_div(rows, kAdaChunk), channels, dweight, dbias);
  return launch_status();
}

int wcn_permute_add(const void* y, const int64_t* index, const void* residual, const float* scale, int32_t scale_at_source,
                    int64_t rows, int32_t channels, int32_t dtype, void* out, wcn_stream_t stream) {
  int st = ln_check(rows, channels, dtype, 0, nullptr, nullptr);
  if ((st == WCN_SUCCESS || st == 1) && scale_at_source != 0 && scale_at_source != 1) st = WCN_ERROR_INVALID_PARAMETERS;
  if (st == WCN_SUCCESS) {
    if (!y || !index || !out) st = WCN_ERROR_INVALID_PARAMETERS;
    else if (!aligned_to(y, 16) || !aligned_to(index, 8) || !aligned_to(residual, 16) || !aligned_to(scale, 4) ||
             !aligned_to(out, 16))
      st = WCN_ERROR_INVALID_PARAMETERS;
  }
  if (st != WCN_SUCCESS) return st == 1 ? WCN_SUCCESS : st;
  PermGeom g;
  g.rows = rows;
  g.units = 0;
  g.channels = channels;
  g.glog = row_glog(channels / 8);
  g.scale_at_source = scale_at_source;
  return with_dtype(dtype, [&](auto el) {
    return permute_add_t<decltype(el)>(y, index, residual, scale, out, g, (hipStream_t)stream);
  });
}

int wcn_channel_spread(const void* x, const void* h, int64_t rows, int32_t cx, int32_t r, float alpha, int32_t dtype,
                       void* out, wcn_stream_t stream) {
  return skip_run(false, x, h, rows, cx, r, alpha, dtype, out, (hipStream_t)stream);
}

int wcn_channel_fold(const void* x, const void* h, int64_t rows, int32_t cout, int32_t g, float alpha, int32_t dtype,
                     void* out, wcn_stream_t stream) {
  return skip_run(true, x, h, rows, cout, g, alpha, dtype, out, (hipStream_t)stream);
}
