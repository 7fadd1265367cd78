// adaln.hip - the per-voxel glue of an adaLN-modulated sparse transformer block (reference: nn/modules/sparse_dit.py:108-123
// runs it as a dozen element-wise torch passes per branch: x.float(), the norm, the cast back, three t[batch_index] gathers
// that write [T, C] copies of the per-batch vectors, 1 +, two multiplies, two adds).  One row-streaming kernel family per
// direction, two compile-time switches:
//   RES   x1 = x + h * gate[b]                         (the gated residual; x1 is written, rounded once)
//   NORM  y  = LN(x1) * (1 + scale[b]) + shift[b]      (LN without affine parameters, biased variance, from the fp32 x1)
// so that NORM alone opens a block, RES + NORM sits between the attention and the MLP, and RES alone closes it.  b is the
// segment of the row: cu[b] <= t < cu[b+1], cu int32 [B + 1] on the device, empty segments allowed, never read on the host.
// shift / scale / gate are fp32 [B, C] views with one row pitch (chunks of one [B, 6C] tensor).
//
// Launch shape and row arithmetic are ada_row.h's, shared with ln_act.hip: G lanes stand side by side on a row and hold
// it in registers, NCH <= 4 pieces of 8 elements each; row sums cross the G lanes with an xor butterfly; the variance is
// two-pass.  Here is what is adaLN's own: the gated residual in front of the statistics, 1 + scale and shift behind them,
// the segment of a row and the per-segment column sums.
//   forward   the lane groups stride over the rows; writes stats [T, 2] = (mean, rstd) for the backward.
//   backward  reads x, not the rounded x1 the forward wrote: x1 = x + h * gate[b] is formed again in fp32, so xhat is the
//             forward's at the same bytes per element.  Lane group u owns the chunk of kAdaChunk consecutive rows u and
//             keeps the column sums of dgate / dshift / dscale in registers.  Where the segment changes inside the chunk,
//             and at its end, the sums go to the partial slot u + b: every (chunk, segment) pair with a row has its own
//             slot, slots grow along the rows, and segment b
//             owns the contiguous slots [cu[b] / R + b, (cu[b+1] - 1) / R + b].  adaln_final_kernel adds each segment's
//             slots in a fixed order.  No float atomics, no zero-filled workspace: two runs are bit-identical.
#include <limits.h>

#include "ada_row.h"

namespace wcn {

struct AdaGeom {
  int64_t rows;   // T
  int64_t units;  // lane groups of the launch: the forward's stride over the rows, the backward's chunks
  int64_t mod_ld;
  int channels, num_segs, glog;
  float eps;
};

template <typename T, int NCH, bool NORM, bool RES>
__global__ __launch_bounds__(kAdaThreads) void adaln_fwd_kernel(const T* __restrict__ x, const T* __restrict__ h,
                                                                const float* __restrict__ gate, const float* __restrict__ shift,
                                                                const float* __restrict__ scale, const int32_t* __restrict__ cu,
                                                                T* __restrict__ x1, T* __restrict__ y,
                                                                float* __restrict__ stats, const AdaGeom g) {
  const RowLane l = row_lane(g.glog, g.channels);
  const int C = g.channels;
  const float fc = (float)C;

  // every lane of a wave walks the same number of trips: the butterfly needs its partners
  for (int64_t t0 = 0; t0 < g.rows; t0 += g.units) {
    const int64_t t = t0 + l.unit;
    const bool act = t < g.rows;
    const int b = act ? last_offset_not_above(cu, g.num_segs, t) : 0;
    float f[NCH][8];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * l.G;
      if (act && c < l.nvec) {
        const int64_t at = t * C + c * 8;
        ld_vec(x + at, f[k]);
        if constexpr (RES) {
          float hv[8], gv[8];
          ld_vec(h + at, hv);
          ld_vec(gate + b * g.mod_ld + c * 8, gv);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[k][e] += hv[e] * gv[e];
          st_vec(x1 + at, f[k]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s += f[k][e];
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[k][e] = 0.f;
      }
    }
    if constexpr (NORM) {
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
          float sc[8], sh[8], o[8];
          ld_vec(scale + b * g.mod_ld + c * 8, sc);
          ld_vec(shift + b * g.mod_ld + c * 8, sh);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (f[k][e] - st.delta) * st.rstd * (1.0f + sc[e]) + sh[e];
          st_vec(y + t * C + c * 8, o);
        }
      }
    }
  }
}

// partial [slots][3][C]: 0 = dgate, 1 = dshift, 2 = dscale
template <typename T, int NCH, bool NORM, bool RES>
__global__ __launch_bounds__(kAdaThreads) void adaln_bwd_kernel(const T* __restrict__ dx1, const T* __restrict__ dy,
                                                                const T* __restrict__ x, const T* __restrict__ h,
                                                                const float* __restrict__ gate, const float* __restrict__ scale,
                                                                const float* __restrict__ stats, const int32_t* __restrict__ cu,
                                                                T* __restrict__ dx, T* __restrict__ dh,
                                                                float* __restrict__ partial, const AdaGeom g) {
  const RowLane l = row_lane(g.glog, g.channels);
  const int C = g.channels;
  const float inv_c = 1.0f / (float)C;
  const bool live = l.unit < g.units;
  const bool has_dx1 = dx1 != nullptr;  // the same in every lane

  float a_gate[RES ? NCH : 1][8], a_shift[NORM ? NCH : 1][8], a_scale[NORM ? NCH : 1][8];
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if constexpr (RES) a_gate[k][e] = 0.f;
      if constexpr (NORM) { a_shift[k][e] = 0.f; a_scale[k][e] = 0.f; }
    }

  // the lane's sums -> slot unit + seg, then zero
  auto flush = [&](int seg) {
    float* p = partial + (l.unit + seg) * 3 * (int64_t)C;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * l.G;
      if (c < l.nvec) {
        if constexpr (RES) st_vec(p + c * 8, a_gate[k]);
        if constexpr (NORM) { st_vec(p + C + c * 8, a_shift[k]); st_vec(p + 2 * C + c * 8, a_scale[k]); }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if constexpr (RES) a_gate[k][e] = 0.f;
        if constexpr (NORM) { a_shift[k][e] = 0.f; a_scale[k][e] = 0.f; }
      }
    }
  };

  int b = -1;              // segment of the rows summed so far; -1: none yet
  int64_t next = 0;        // cu[b + 1], or never
#pragma unroll 1
  for (int i = 0; i < kAdaChunk; ++i) {
    const int64_t t = l.unit * kAdaChunk + i;
    const bool act = live && t < g.rows;
    if (act) {
      int nb = b;
      if (nb < 0) {
        nb = last_offset_not_above(cu, g.num_segs, t);
        next = nb + 1 < g.num_segs ? (int64_t)cu[nb + 1] : LLONG_MAX;
      } else {
        while (t >= next) {  // ends at the last segment at the latest
          ++nb;
          next = nb + 1 < g.num_segs ? (int64_t)cu[nb + 1] : LLONG_MAX;
        }
      }
      if (nb != b) {
        if (b >= 0) flush(b);
        b = nb;
      }
    }
    const int bb = b < 0 ? 0 : b;
    float gd[NCH][8], xh[NCH][8];  // g = dy (1 + scale); xhat
    float hk[NORM && RES ? NCH : 1][8];
    float mean = 0.f, rstd = 0.f, s1 = 0.f, s2 = 0.f;
    if constexpr (NORM) {
      if (act) row_stats_ld(stats, t, mean, rstd);
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        const int c = l.gl + k * l.G;
        if (act && c < l.nvec) {
          const int64_t at = t * C + c * 8;
          float xv[8], sc[8];
          ld_vec(dy + at, gd[k]);
          ld_vec(x + at, xv);
          if constexpr (RES) {  // what LN read is the forward's fp32 x1, formed again with the same operations
            float gv[8];
            ld_vec(h + at, hk[k]);
            ld_vec(gate + bb * g.mod_ld + c * 8, gv);
#pragma unroll
            for (int e = 0; e < 8; ++e) xv[e] += hk[k][e] * gv[e];
          }
          ld_vec(scale + bb * g.mod_ld + c * 8, sc);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float d = gd[k][e];
            xh[k][e] = row_xhat(xv[e], mean, rstd);
            a_shift[k][e] += d;
            a_scale[k][e] += d * xh[k][e];
            gd[k][e] = d * (1.0f + sc[e]);
            s1 += gd[k][e];
            s2 += gd[k][e] * xh[k][e];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) { gd[k][e] = 0.f; xh[k][e] = 0.f; }
        }
      }
      s1 = row_mean_rcp(s1, g.glog, inv_c);
      s2 = row_mean_rcp(s2, g.glog, inv_c);
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * l.G;
      if (act && c < l.nvec) {
        const int64_t at = t * C + c * 8;
        float r[8];
        if (has_dx1) {
          ld_vec(dx1 + at, r);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) r[e] = 0.f;
        }
        if constexpr (NORM) {
#pragma unroll
          for (int e = 0; e < 8; ++e) r[e] += row_dx(rstd, gd[k][e], xh[k][e], s1, s2);
        }
        if (NORM || dx != nullptr) st_vec(dx + at, r);
        if constexpr (RES) {
          float hv[8], gv[8], o[8];
          if constexpr (NORM) {
#pragma unroll
            for (int e = 0; e < 8; ++e) hv[e] = hk[k][e];
          } else {
            ld_vec(h + at, hv);
          }
          ld_vec(gate + bb * g.mod_ld + c * 8, gv);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            o[e] = r[e] * gv[e];
            a_gate[k][e] += r[e] * hv[e];
          }
          st_vec(dh + at, o);
        }
      }
    }
  }
  if (b >= 0) flush(b);
}

// second level of the column sums: 32 columns x 8 slot slices per workgroup, one segment and one of the three sums each;
// both levels in a fixed order.  A segment without rows gets zeros.
__global__ __launch_bounds__(256) void adaln_final_kernel(const float* __restrict__ partial, const int32_t* __restrict__ cu,
                                                          int64_t rows, int C, float* __restrict__ dgate,
                                                          float* __restrict__ dshift, float* __restrict__ dscale,
                                                          int64_t out_ld) {
  __shared__ float s[8][33];
  const int which = blockIdx.z;
  float* out = which == 0 ? dgate : which == 1 ? dshift : dscale;
  if (out == nullptr) return;  // the whole workgroup
  const int64_t b = blockIdx.x;
  const int cl = threadIdx.x & 31, q = threadIdx.x >> 5;
  const int col = blockIdx.y * 32 + cl;
  int64_t lo = cu[b], hi = cu[b + 1];
  lo = lo < 0 ? 0 : lo > rows ? rows : lo;
  hi = hi < 0 ? 0 : hi > rows ? rows : hi;
  float sum = 0.f;
  if (col < C && hi > lo) {
    const int64_t first = lo / kAdaChunk + b, last = (hi - 1) / kAdaChunk + b;
    for (int64_t sl = first + q; sl <= last; sl += 8) sum += partial[(sl * 3 + which) * C + col];
  }
  s[q][cl] = sum;
  __syncthreads();
  if (q == 0 && col < C) {
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) tot += s[i][cl];
    out[b * out_ld + col] = tot;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
static AdaGeom ada_geom(int64_t rows, int64_t num_segs, int channels, int64_t mod_ld, float eps) {
  AdaGeom g;
  g.rows = rows;
  g.units = 0;
  g.mod_ld = mod_ld;
  g.channels = channels;
  g.num_segs = (int)num_segs;
  g.glog = row_glog(channels / 8);
  g.eps = eps;
  return g;
}

// Shared argument checks.  Returns WCN_SUCCESS, an error, or 1 = valid but nothing to launch.
static int ada_check(int64_t rows, int64_t num_segs, int32_t channels, int32_t dtype, bool norm, bool res, bool paired,
                     int64_t mod_ld) {
  if (rows < 0 || num_segs < 0) return WCN_ERROR_INVALID_PARAMETERS;
  if (!wcn_adaln_supported(channels, dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if ((!norm && !res) || !paired) return WCN_ERROR_INVALID_PARAMETERS;
  if (rows > INT32_MAX || num_segs > INT32_MAX) return WCN_ERROR_INVALID_PARAMETERS;  // cu is int32
  if (mod_ld < channels || mod_ld % 4 != 0) return WCN_ERROR_INVALID_PARAMETERS;      // 16-B pieces of the fp32 rows
  return rows == 0 || num_segs == 0 ? 1 : WCN_SUCCESS;
}

template <typename T, bool NORM, bool RES>
static int ada_fwd_t(const void* x, const void* h, const float* gate, const float* shift, const float* scale,
                     const int32_t* cu, void* x1, void* y, float* stats, AdaGeom g, hipStream_t s) {
  const unsigned blocks = row_fwd_grid(g.rows, g.glog, &g.units);
  row_with_nch(g.channels, g.glog, [&](auto nch) {
    hipLaunchKernelGGL((adaln_fwd_kernel<T, nch(), NORM, RES>), dim3(blocks), dim3(kAdaThreads), 0, s, (const T*)x,
                       (const T*)h, gate, shift, scale, cu, (T*)x1, (T*)y, stats, g);
  });
  return launch_status();
}

template <typename T, bool NORM, bool RES>
static int ada_bwd_t(const void* dx1, const void* dy, const void* x, const void* h, const float* gate, const float* scale,
                     const float* stats, const int32_t* cu, void* dx, void* dh, float* partial, AdaGeom g, hipStream_t s) {
  const unsigned blocks = row_bwd_grid(g.rows, g.glog, &g.units);
  row_with_nch(g.channels, g.glog, [&](auto nch) {
    hipLaunchKernelGGL((adaln_bwd_kernel<T, nch(), NORM, RES>), dim3(blocks), dim3(kAdaThreads), 0, s, (const T*)dx1,
                       (const T*)dy, (const T*)x, (const T*)h, gate, scale, stats, cu, (T*)dx, (T*)dh, partial, g);
  });
  return launch_status();
}

// the three uses of one dtype
#define WCN_ADA_USES(FN, T, ...)                                      \
  (norm && res ? FN<T, true, true>(__VA_ARGS__)                       \
               : norm ? FN<T, true, false>(__VA_ARGS__) : FN<T, false, true>(__VA_ARGS__))
#define WCN_ADA_DTYPES(FN, ...) \
  with_dtype(dtype, [&](auto el) { return WCN_ADA_USES(FN, decltype(el), __VA_ARGS__); })

}  // namespace wcn

using namespace wcn;

int wcn_adaln_supported(int32_t channels, int32_t dtype) {
  return channels >= 8 && channels % 8 == 0 && channels <= kAdaMaxChannels && dtype_ok(dtype) ? 1 : 0;
}

size_t wcn_adaln_workspace_bytes(int64_t rows, int64_t num_segs, int32_t channels) {
  if (rows <= 0 || num_segs <= 0 || channels < 1) return 0;
  return (size_t)(ceil_div(rows, kAdaChunk) + num_segs) * 3 * (size_t)channels * sizeof(float);
}

int wcn_adaln_fwd(const void* x, const void* h, const float* gate, const float* shift, const float* scale, int64_t mod_ld,
                  const int32_t* cu, int64_t num_segs, int64_t rows, int32_t channels, float eps, int32_t dtype, void* x1,
                  void* y, float* stats, wcn_stream_t stream) {
  const bool res = h != nullptr || gate != nullptr, norm = shift != nullptr || scale != nullptr;
  const bool paired = (h != nullptr) == (gate != nullptr) && (shift != nullptr) == (scale != nullptr);
  int st = ada_check(rows, num_segs, channels, dtype, norm, res, paired, mod_ld);
  if ((st == WCN_SUCCESS || st == 1) && !(eps >= 0.f)) st = WCN_ERROR_INVALID_PARAMETERS;
  if (st == WCN_SUCCESS) {
    if (!x || !cu || (res && !x1) || (norm && (!y || !stats))) st = WCN_ERROR_INVALID_PARAMETERS;
    else if (!aligned_to(x, 16) || !aligned_to(h, 16) || !aligned_to(gate, 16) || !aligned_to(shift, 16) ||
             !aligned_to(scale, 16) || !aligned_to(x1, 16) || !aligned_to(y, 16) || !aligned_to(stats, 8) ||
             !aligned_to(cu, 4))
      st = WCN_ERROR_INVALID_PARAMETERS;
  }
  if (st != WCN_SUCCESS) return st == 1 ? WCN_SUCCESS : st;
  const AdaGeom g = ada_geom(rows, num_segs, channels, mod_ld, eps);
  return WCN_ADA_DTYPES(ada_fwd_t, x, h, gate, shift, scale, cu, x1, y, stats, g, (hipStream_t)stream);
}

int wcn_adaln_bwd(const void* dx1, const void* dy, const void* x, const void* h, const float* gate, const float* scale,
                  int64_t mod_ld, const float* stats, const int32_t* cu, int64_t num_segs, int64_t rows, int32_t channels,
                  int32_t dtype, void* dx, void* dh, float* dgate, float* dshift, float* dscale, int64_t dmod_ld,
                  void* workspace, size_t workspace_bytes, wcn_stream_t stream) {
  const bool res = h != nullptr || gate != nullptr, norm = dy != nullptr || scale != nullptr;
  const bool paired = (h != nullptr) == (gate != nullptr) && (dy != nullptr) == (scale != nullptr);
  int st = ada_check(rows, num_segs, channels, dtype, norm, res, paired, mod_ld);
  if ((st == WCN_SUCCESS || st == 1) &&
      (dmod_ld < channels || workspace_bytes < wcn_adaln_workspace_bytes(rows, num_segs, channels)))
    st = WCN_ERROR_INVALID_PARAMETERS;
  if ((st == WCN_SUCCESS || st == 1) && num_segs > 0 && ((res && !dgate) || (norm && (!dshift || !dscale))))
    st = WCN_ERROR_INVALID_PARAMETERS;
  if (st == WCN_SUCCESS) {
    if (!cu || !workspace || (!norm && !dx1) || (norm && (!x || !stats || !dx)) || (res && !dh)) st = WCN_ERROR_INVALID_PARAMETERS;
    else if (!aligned_to(dx1, 16) || !aligned_to(dy, 16) || !aligned_to(x, 16) || !aligned_to(h, 16) ||
             !aligned_to(gate, 16) || !aligned_to(scale, 16) || !aligned_to(stats, 8) || !aligned_to(cu, 4) ||
             !aligned_to(dx, 16) || !aligned_to(dh, 16) || !aligned_to(dgate, 4) || !aligned_to(dshift, 4) ||
             !aligned_to(dscale, 4) || !aligned_to(workspace, 16))
      st = WCN_ERROR_INVALID_PARAMETERS;
  }
  hipStream_t s = (hipStream_t)stream;
  if (st == 1) {  // no rows: every segment's sums are zero, and no kernel runs
    if (num_segs > 0) {
      float* outs[3] = {res ? dgate : nullptr, norm ? dshift : nullptr, norm ? dscale : nullptr};
      for (float* o : outs)
        if (o && hipMemset2DAsync(o, (size_t)dmod_ld * sizeof(float), 0, (size_t)channels * sizeof(float), (size_t)num_segs,
                                  s) != hipSuccess)
          return WCN_ERROR_KERNEL_EXECUTION;
    }
    return WCN_SUCCESS;
  }
  if (st != WCN_SUCCESS) return st;
  const AdaGeom g = ada_geom(rows, num_segs, channels, mod_ld, 0.f);
  float* partial = (float*)workspace;
  st = WCN_ADA_DTYPES(ada_bwd_t, dx1, dy, x, h, gate, scale, stats, cu, dx, dh, partial, g, s);
  if (st != WCN_SUCCESS) return st;
  hipLaunchKernelGGL(adaln_final_kernel, dim3((unsigned)num_segs, (unsigned)ceil_div(channels, 32), 3), dim3(256), 0, s,
                     (const float*)partial, cu, rows, channels, res ? dgate : nullptr, norm ? dshift : nullptr,
                     norm ? dscale : nullptr, dmod_ld);
  return launch_status();
}
