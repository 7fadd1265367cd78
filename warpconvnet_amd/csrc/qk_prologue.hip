// qk_prologue.hip - the Q/K prologue of sparse voxel self-attention: per-head RMS norm of Q and K, rotary position
// embedding from the voxel coordinates, and the cast to the attention core's dtype, as ONE streaming pass over the packed
// qkv tensor [T, 3, H, D] (reference: nn/modules/sparse_dit_attention.py:249-262 runs unbind -> MultiHeadRMSNorm ->
// _rotary_embedding -> stack as eight-odd torch passes; csrc/fused_rope_kernel.cu is its hand-written rotation).
//
// The rotation (one definition for both reference conventions).  A head of width D (even) is D / 2 pairs
// (x[2j], x[2j+1]).  Pair j < rot_pairs = 3 F turns by the angle pos[a] * freqs[f], a = j / F, f = j % F,
// pos[a] = float(coord[a]) - origin[a] + bias (fp32, one rounding per operation); pairs j >= 3 F and the whole V slot pass
// through.  out = (x0 cos - x1 sin, x0 sin + x1 cos); conjugate = 1 negates sin (the inverse rotation = the backward).
//   wcn_rope_table       (cos, sin) of every (token, pair) once, with the accurate sincosf: table [T, 3F, 2] fp32.  The
//                        same entries serve every head, Q and K, every block that shares the coordinates, and the backward,
//                        so the hot kernels hold no trigonometry.
//   wcn_qk_prologue_fwd  y = x / max(|x|_2, 1e-12) * gamma[h] * sqrt(D) per (token, head) of Q and K (optional), then
//                        the rotation (optional), then one rounding to the output dtype; V is copied (cast).
//   wcn_qk_prologue_bwd  the inverse rotation of dout, then the norm's backward; dgamma through per-row-group partial
//                        sums in a caller workspace and a fixed-order second pass (no float atomics: two runs are
//                        bit-identical).
//
// Launch shape.  A (token, slot, head) is D contiguous elements, a token row 3 H D of them.  G = the power of two >=
// D / EPL lanes stand side by side on one (slot, head), EPL elements each: 16 bytes (8 x f16 / bf16, 4 x f32 - whole
// pairs, whose (cos, sin) entries are contiguous in the table) when D is a multiple of that, else the generic path with
// one pair per lane and up to two chunks per lane (any even D <= 256).  L = 3 H G lanes cover a row; `rows` row groups
// run side by side and stride over the tokens, so a workgroup reads consecutive rows and a lane keeps ONE column for the
// whole launch: its gamma is loaded once, and in the backward its dgamma terms add up in registers.  The sum of squares
// of a head goes across its G lanes with an xor butterfly of lane permutes (every lane ends with the same bits).  No LDS,
// no atomics, no scratch in the streaming kernels.
#include <math.h>

#include "wcn_common.h"

namespace wcn {

constexpr int kQkMaxHeadDim = 256;
constexpr float kQkNormEps = 1e-12f;
constexpr int kQkThreads = 256;
constexpr int kQkLaneBudget = 1 << 19;  // lanes in flight the row groups are sized for (2048 workgroups of 256)


struct QkGeom {
  int64_t total;           // T
  int heads, head_dim;
  int rot_pairs;           // 3 F; 0 = no rotation
  int group;               // G lanes per (slot, head), a power of two <= 64
  int rows;                // row groups side by side
  uint32_t lanes_per_row;  // L = 3 H G
};

// Row groups of a launch.  A function of (T, H, D) alone - not of the dtypes - because it also sizes the backward's workspace.
static int qk_rows(int64_t total, int heads, int head_dim) {
  const int64_t nominal = (int64_t)3 * heads * (head_dim >= 8 ? head_dim / 8 : 1);
  int64_t r = kQkLaneBudget / nominal;
  if (r < 1) r = 1;
  return (int)(r < total ? r : total);
}

// The lane's place: row group, (slot, head), lane within the group.
struct QkLane {
  uint32_t row;
  int slot, head, gl;
  bool live;
};
__device__ __forceinline__ QkLane qk_lane(const QkGeom& g) {
  QkLane l;
  const uint32_t v = blockIdx.x * (uint32_t)kQkThreads + threadIdx.x;
  l.row = v / g.lanes_per_row;
  const uint32_t col = v - l.row * g.lanes_per_row;
  const uint32_t sh = col / (uint32_t)g.group;
  l.gl = (int)(col - sh * (uint32_t)g.group);
  l.slot = (int)(sh / (uint32_t)g.heads);
  l.head = (int)(sh - (uint32_t)l.slot * (uint32_t)g.heads);
  l.live = l.row < (uint32_t)g.rows;
  return l;
}

// sum over the G lanes of a group; every lane of the group receives the same bits
__device__ __forceinline__ float qk_group_sum(float v, int group) {
  for (int m = 1; m < group; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// rotate the pairs of one chunk in place; `pair0` = index of the chunk's first pair within the head
template <int EPL>
__device__ __forceinline__ void qk_rotate(float (&f)[EPL], const float* __restrict__ trow, int pair0, int rot_pairs, float sgn) {
#pragma unroll
  for (int p = 0; p < EPL / 2; ++p) {
    if (pair0 + p < rot_pairs) {
      const float2 cs = *reinterpret_cast<const float2*>(trow + 2 * (pair0 + p));
      const float c = cs.x, s = sgn * cs.y;
      const float x0 = f[2 * p], x1 = f[2 * p + 1];
      f[2 * p] = x0 * c - x1 * s;
      f[2 * p + 1] = x0 * s + x1 * c;
    }
  }
}

template <typename TI, typename TO, int EPL, int NCH>
__global__ __launch_bounds__(kQkThreads) void qk_fwd_kernel(const TI* __restrict__ x, TO* __restrict__ out,
                                                            const float* __restrict__ table,
                                                            const float* __restrict__ gamma_q,
                                                            const float* __restrict__ gamma_k,
                                                            float* __restrict__ inv_norm, const QkGeom g, int conjugate) {
  const QkLane l = qk_lane(g);
  const int D = g.head_dim, nchunk = D / EPL;
  const bool has_norm = gamma_q != nullptr;  // the same in every lane
  const bool qk = l.slot < 2;
  const float sgn = conjugate ? -1.f : 1.f;
  const float sqrt_d = sqrtf((float)D);
  const int64_t row_elems = (int64_t)3 * g.heads * D;
  const int64_t col0 = ((int64_t)l.slot * g.heads + l.head) * D;

  bool mine[NCH];
  float gam[NCH][EPL];
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = l.gl + k * g.group;
    mine[k] = l.live && c < nchunk;
#pragma unroll
    for (int e = 0; e < EPL; ++e) gam[k][e] = 1.f;
    if (has_norm && qk && mine[k]) {
      const float* gp = (l.slot == 0 ? gamma_q : gamma_k) + (int64_t)l.head * D + c * EPL;
#pragma unroll
      for (int e = 0; e < EPL; ++e) gam[k][e] = gp[e] * sqrt_d;
    }
  }

  // every lane of a wave walks the same number of trips: the butterfly needs its partners
  for (int64_t t0 = 0; t0 < g.total; t0 += g.rows) {
    const int64_t t = t0 + l.row;
    const bool act = t < g.total;
    float f[NCH][EPL];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * g.group;
      if (mine[k] && act) {
        ld_vec(x + t * row_elems + col0 + c * EPL, f[k]);
#pragma unroll
        for (int e = 0; e < EPL; ++e) ss += f[k][e] * f[k][e];
      } else {
#pragma unroll
        for (int e = 0; e < EPL; ++e) f[k][e] = 0.f;
      }
    }
    if (has_norm) {
      ss = qk_group_sum(ss, g.group);
      const float inv = 1.0f / fmaxf(sqrtf(ss), kQkNormEps);
      if (qk) {
#pragma unroll
        for (int k = 0; k < NCH; ++k)
#pragma unroll
          for (int e = 0; e < EPL; ++e) f[k][e] = f[k][e] * inv * gam[k][e];
        if (l.gl == 0 && l.live && act) inv_norm[(t * 2 + l.slot) * g.heads + l.head] = inv;
      }
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * g.group;
      if (mine[k] && act) {
        if (qk && g.rot_pairs > 0) qk_rotate<EPL>(f[k], table + t * (2 * (int64_t)g.rot_pairs), c * (EPL / 2), g.rot_pairs, sgn);
        Vec<TO, EPL> o;  // not st_vec, nor ld_vec for x in the backward: the compiler orders and allocates them differently
#pragma unroll
        for (int e = 0; e < EPL; ++e) o.v[e] = (TO)f[k][e];
        *reinterpret_cast<Vec<TO, EPL>*>(out + t * row_elems + col0 + c * EPL) = o;
      }
    }
  }
}

// Backward with the norm: dy = inverse rotation of dout; u = gamma sqrt(D) dy; xh = x inv_norm;
// dx = (u - xh (xh . u)) inv_norm, or u / 1e-12 where the norm was clamped; dgamma[h, d] += sqrt(D) xh dy, kept in the
// lane's registers over all its tokens and written once to partial [rows][2][H][D].
template <typename TX, typename TG, int EPL, int NCH>
__global__ __launch_bounds__(kQkThreads) void qk_bwd_kernel(const TG* __restrict__ dout, const TX* __restrict__ x,
                                                            TX* __restrict__ dx, const float* __restrict__ table,
                                                            const float* __restrict__ gamma_q,
                                                            const float* __restrict__ gamma_k,
                                                            const float* __restrict__ inv_norm,
                                                            float* __restrict__ partial, const QkGeom g) {
  const QkLane l = qk_lane(g);
  const int D = g.head_dim, nchunk = D / EPL;
  const bool qk = l.slot < 2;
  const float sqrt_d = sqrtf((float)D);
  const float inv_clamped = 1.0f / kQkNormEps;
  const int64_t row_elems = (int64_t)3 * g.heads * D;
  const int64_t col0 = ((int64_t)l.slot * g.heads + l.head) * D;

  bool mine[NCH];
  float gam[NCH][EPL], acc[NCH][EPL];
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = l.gl + k * g.group;
    mine[k] = l.live && c < nchunk;
#pragma unroll
    for (int e = 0; e < EPL; ++e) { gam[k][e] = 0.f; acc[k][e] = 0.f; }
    if (qk && mine[k]) {
      const float* gp = (l.slot == 0 ? gamma_q : gamma_k) + (int64_t)l.head * D + c * EPL;
#pragma unroll
      for (int e = 0; e < EPL; ++e) gam[k][e] = gp[e] * sqrt_d;
    }
  }

  for (int64_t t0 = 0; t0 < g.total; t0 += g.rows) {
    const int64_t t = t0 + l.row;
    const bool act = t < g.total;
    float dy[NCH][EPL], xh[NCH][EPL];
    float inv = 0.f, dot = 0.f;
    if (qk && l.live && act) inv = inv_norm[(t * 2 + l.slot) * g.heads + l.head];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * g.group;
      if (mine[k] && act) {
        const int64_t at = t * row_elems + col0 + c * EPL;
        ld_vec(dout + at, dy[k]);
        if (qk) {
          const Vec<TX, EPL> xv = *reinterpret_cast<const Vec<TX, EPL>*>(x + at);
          if (g.rot_pairs > 0) qk_rotate<EPL>(dy[k], table + t * (2 * (int64_t)g.rot_pairs), c * (EPL / 2), g.rot_pairs, -1.f);
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            xh[k][e] = (float)xv.v[e] * inv;
            acc[k][e] += xh[k][e] * dy[k][e];  // sqrt(D) is applied once, at the end
            dy[k][e] *= gam[k][e];             // u
            dot += xh[k][e] * dy[k][e];
          }
        } else {
#pragma unroll
          for (int e = 0; e < EPL; ++e) xh[k][e] = 0.f;
        }
      } else {
#pragma unroll
        for (int e = 0; e < EPL; ++e) { dy[k][e] = 0.f; xh[k][e] = 0.f; }
      }
    }
    dot = qk_group_sum(dot, g.group);
    if (inv >= inv_clamped) dot = 0.f;  // the clamped norm is a constant: dx = u / 1e-12
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = l.gl + k * g.group;
      if (mine[k] && act) {
        float o[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) o[e] = qk ? (dy[k][e] - xh[k][e] * dot) * inv : dy[k][e];
        st_vec(dx + t * row_elems + col0 + c * EPL, o);
      }
    }
  }

#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = l.gl + k * g.group;
    if (qk && mine[k]) {
      float* p = partial + (((int64_t)l.row * 2 + l.slot) * g.heads + l.head) * D + c * EPL;
#pragma unroll
      for (int e = 0; e < EPL; ++e) p[e] = acc[k][e] * sqrt_d;
    }
  }
}

// second level of dgamma: 16 columns x 16 row slices per workgroup, both levels summed in a fixed order
__global__ __launch_bounds__(256) void qk_dgamma_final_kernel(const float* __restrict__ partial, int rows, int hd,
                                                              float* __restrict__ dgamma_q, float* __restrict__ dgamma_k) {
  __shared__ float s[16][17];
  const int cl = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + cl, ncols = 2 * hd;
  float sum = 0.f;
  if (col < ncols)
    for (int r = q; r < rows; r += 16) sum += partial[(int64_t)r * ncols + col];
  s[q][cl] = sum;
  __syncthreads();
  if (q == 0 && col < ncols) {
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) tot += s[i][cl];
    if (col < hd) dgamma_q[col] = tot; else dgamma_k[col - hd] = tot;
  }
}

template <typename TC>
__global__ __launch_bounds__(256) void rope_table_kernel(const TC* __restrict__ coords, const float* __restrict__ origin,
                                                         float bias, const float* __restrict__ freqs, int nfreq,
                                                         int64_t entries, float* __restrict__ table) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= entries) return;
  const int pairs = 3 * nfreq;
  const int64_t t = i / pairs;
  const int j = (int)(i - t * pairs);
  const int a = j / nfreq, f = j - a * nfreq;
  float pos = (float)coords[t * 3 + a];
  pos = pos - (origin ? origin[a] : 0.f);
  pos = pos + bias;
  const float ang = pos * freqs[f];
  float sn, cs;
  sincosf(ang, &sn, &cs);  // the accurate one: angles reach thousands of radians
  reinterpret_cast<float2*>(table)[i] = make_float2(cs, sn);
}

// The axial table: axis a owns its own frequency count; pair j of a token belongs to the axis whose run of the concatenated
// frequency vector holds j.  Same operations, same order as rope_table_kernel.
struct RopeAxes {
  int n0, n1, n2;
};
template <typename TC>
__global__ __launch_bounds__(256) void rope_table_axes_kernel(const TC* __restrict__ coords, const float* __restrict__ origin,
                                                              float bias, const float* __restrict__ freqs, RopeAxes ax,
                                                              int64_t entries, float* __restrict__ table) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= entries) return;
  const int pairs = ax.n0 + ax.n1 + ax.n2;
  const int64_t t = i / pairs;
  const int j = (int)(i - t * pairs);
  const int a = j < ax.n0 ? 0 : (j < ax.n0 + ax.n1 ? 1 : 2);
  float pos = (float)coords[t * 3 + a];
  pos = pos - (origin ? origin[a] : 0.f);
  pos = pos + bias;
  const float ang = pos * freqs[j];  // (freqs is the concatenation: entry j is axis a's own frequency)
  float sn, cs;
  sincosf(ang, &sn, &cs);
  reinterpret_cast<float2*>(table)[i] = make_float2(cs, sn);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
static int qk_pow2_ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

// The path of a launch: 16-B lanes when D and the buffers allow it, else one pair per lane.
struct QkPath {
  int epl, nch;
  QkGeom g;
};
static QkPath qk_path(int64_t total, int heads, int head_dim, int rot_pairs, int size_a, int size_b, bool aligned16) {
  QkPath p;
  const int vec = 16 / (size_a > size_b ? size_a : size_b);
  p.epl = head_dim % vec == 0 && aligned16 ? vec : 2;
  const int nchunk = head_dim / p.epl;
  p.g.group = qk_pow2_ceil(nchunk < 64 ? nchunk : 64);
  p.nch = (nchunk + p.g.group - 1) / p.g.group;
  p.g.total = total;
  p.g.heads = heads;
  p.g.head_dim = head_dim;
  p.g.rot_pairs = rot_pairs;
  p.g.rows = qk_rows(total, heads, head_dim);
  p.g.lanes_per_row = (uint32_t)3 * heads * p.g.group;
  return p;
}
// a lane's piece of the narrower buffer is 8 B, of the wider 16 B: every buffer 16-B aligned covers both
static bool qk_all_aligned16(const void* a, const void* b, const void* c = nullptr) {
  return aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(c, 16);
}
static unsigned qk_grid(const QkGeom& g) { return (unsigned)ceil_div((int64_t)g.rows * g.lanes_per_row, kQkThreads); }

template <typename TI, typename TO>
static int qk_fwd_t(const void* x, void* out, const float* table, const float* gq, const float* gk, float* inv_norm,
                    const QkPath& p, int conjugate, hipStream_t s) {
  constexpr int kVec = 16 / (sizeof(TI) > sizeof(TO) ? sizeof(TI) : sizeof(TO));
#define WCN_QK_FWD(EPL, NCH)                                                                                              \
  hipLaunchKernelGGL((qk_fwd_kernel<TI, TO, EPL, NCH>), dim3(qk_grid(p.g)), dim3(kQkThreads), 0, s, (const TI*)x, (TO*)out, \
                     table, gq, gk, inv_norm, p.g, conjugate)
  if (p.epl == kVec) WCN_QK_FWD(kVec, 1);
  else if (p.nch == 1) WCN_QK_FWD(2, 1);
  else WCN_QK_FWD(2, 2);
#undef WCN_QK_FWD
  return launch_status();
}

template <typename TX, typename TG>
static int qk_bwd_t(const void* dout, const void* x, void* dx, const float* table, const float* gq, const float* gk,
                    const float* inv_norm, float* partial, const QkPath& p, hipStream_t s) {
  constexpr int kVec = 16 / (sizeof(TX) > sizeof(TG) ? sizeof(TX) : sizeof(TG));
#define WCN_QK_BWD(EPL, NCH)                                                                                               \
  hipLaunchKernelGGL((qk_bwd_kernel<TX, TG, EPL, NCH>), dim3(qk_grid(p.g)), dim3(kQkThreads), 0, s, (const TG*)dout,        \
                     (const TX*)x, (TX*)dx, table, gq, gk, inv_norm, partial, p.g)
  if (p.epl == kVec) WCN_QK_BWD(kVec, 1);
  else if (p.nch == 1) WCN_QK_BWD(2, 1);
  else WCN_QK_BWD(2, 2);
#undef WCN_QK_BWD
  return launch_status();
}

// in dtype x out dtype of the one-pass kernel (the backward without a norm writes the input's dtype, f32 included)
static int qk_fwd_any(const void* x, int in_dtype, void* out, int out_dtype, const float* table, const float* gq,
                      const float* gk, float* inv_norm, const QkPath& p, int conjugate, hipStream_t s) {
  return with_dtype(in_dtype, [&](auto ti) {
    return with_dtype(out_dtype, [&](auto to) {
      return qk_fwd_t<decltype(ti), decltype(to)>(x, out, table, gq, gk, inv_norm, p, conjugate, s);
    });
  });
}

// Shared argument checks.  Returns WCN_SUCCESS, an error, or 1 = valid but nothing to launch.
static int qk_check(const void* a, int a_dtype, const void* b, int b_dtype, bool b_half_only, int64_t total, int32_t heads,
                    int32_t head_dim, const float* table, int32_t rot_pairs, const float* gq, const float* gk) {
  if (total < 0 || heads < 1 || head_dim < 1 || rot_pairs < 0) return WCN_ERROR_INVALID_PARAMETERS;
  if (!dtype_ok(a_dtype) || !dtype_ok(b_dtype) || (b_half_only && b_dtype == WCN_F32) || head_dim % 2 != 0 ||
      head_dim > kQkMaxHeadDim)
    return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (2 * rot_pairs > head_dim || (gq == nullptr) != (gk == nullptr)) return WCN_ERROR_INVALID_PARAMETERS;
  if (total * 3 * heads > INT32_MAX) return WCN_ERROR_INVALID_PARAMETERS;  // (token, slot, head) triples are counted in 32 bits
  if (total == 0) return 1;
  if (!a || !b || (rot_pairs > 0 && !table)) return WCN_ERROR_INVALID_PARAMETERS;
  // whole pairs are the smallest access; 8-B table entries
  if (!aligned_to(a, 2 * (size_t)dtype_bytes(a_dtype)) || !aligned_to(b, 2 * (size_t)dtype_bytes(b_dtype)) ||
      (table && !aligned_to(table, 8)))
    return WCN_ERROR_INVALID_PARAMETERS;
  return WCN_SUCCESS;
}

}  // namespace wcn

using namespace wcn;

int wcn_qk_prologue_supported(int32_t head_dim, int32_t in_dtype, int32_t out_dtype) {
  return head_dim >= 2 && head_dim % 2 == 0 && head_dim <= kQkMaxHeadDim && dtype_ok(in_dtype) &&
                 (out_dtype == WCN_F16 || out_dtype == WCN_BF16)
             ? 1
             : 0;
}

size_t wcn_qk_prologue_workspace_bytes(int64_t total, int32_t heads, int32_t head_dim) {
  if (total <= 0 || heads < 1 || head_dim < 1) return 0;
  return (size_t)qk_rows(total, heads, head_dim) * 2 * (size_t)heads * (size_t)head_dim * sizeof(float);
}

int wcn_rope_table(const void* coords, int32_t coords_float, int64_t total, const float* origin, float bias,
                   const float* freqs, int32_t num_freqs, float* table, wcn_stream_t stream) {
  if (total < 0 || num_freqs < 0 || !(bias == bias)) return WCN_ERROR_INVALID_PARAMETERS;
  if (coords_float != 0 && coords_float != 1) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (6 * (int64_t)num_freqs > kQkMaxHeadDim) return WCN_ERROR_UNSUPPORTED_CONFIG;
  const int64_t entries = total * 3 * num_freqs;
  if (entries == 0) return WCN_SUCCESS;
  if (!coords || !freqs || !table || !aligned_to(table, 8)) return WCN_ERROR_INVALID_PARAMETERS;
  const int64_t blocks = ceil_div(entries, 256);
  if (blocks > INT32_MAX) return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  if (coords_float)
    hipLaunchKernelGGL((rope_table_kernel<float>), dim3((unsigned)blocks), dim3(256), 0, s, (const float*)coords, origin, bias,
                       freqs, num_freqs, entries, table);
  else
    hipLaunchKernelGGL((rope_table_kernel<int32_t>), dim3((unsigned)blocks), dim3(256), 0, s, (const int32_t*)coords, origin,
                       bias, freqs, num_freqs, entries, table);
  return launch_status();
}

int wcn_rope_table_axes(const void* coords, int32_t coords_float, int64_t total, const float* origin, float bias,
                        const float* freqs, const int32_t counts[3], float* table, wcn_stream_t stream) {
  if (total < 0 || !counts || !(bias == bias)) return WCN_ERROR_INVALID_PARAMETERS;
  if (counts[0] < 0 || counts[1] < 0 || counts[2] < 0) return WCN_ERROR_INVALID_PARAMETERS;
  if (coords_float != 0 && coords_float != 1) return WCN_ERROR_UNSUPPORTED_CONFIG;
  const int64_t pairs = (int64_t)counts[0] + counts[1] + counts[2];
  if (2 * pairs > kQkMaxHeadDim) return WCN_ERROR_UNSUPPORTED_CONFIG;
  const int64_t entries = total * pairs;
  if (entries == 0) return WCN_SUCCESS;
  if (!coords || !freqs || !table || !aligned_to(table, 8)) return WCN_ERROR_INVALID_PARAMETERS;
  const int64_t blocks = ceil_div(entries, 256);
  if (blocks > INT32_MAX) return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  const RopeAxes ax{counts[0], counts[1], counts[2]};
  if (coords_float)
    hipLaunchKernelGGL((rope_table_axes_kernel<float>), dim3((unsigned)blocks), dim3(256), 0, s, (const float*)coords, origin,
                       bias, freqs, ax, entries, table);
  else
    hipLaunchKernelGGL((rope_table_axes_kernel<int32_t>), dim3((unsigned)blocks), dim3(256), 0, s, (const int32_t*)coords, origin,
                       bias, freqs, ax, entries, table);
  return launch_status();
}

int wcn_qk_prologue_fwd(const void* qkv, int32_t in_dtype, int64_t total, int32_t heads, int32_t head_dim, const float* table,
                        int32_t rot_pairs, int32_t conjugate, const float* gamma_q, const float* gamma_k, void* out,
                        int32_t out_dtype, float* inv_norm, wcn_stream_t stream) {
  int st = qk_check(qkv, in_dtype, out, out_dtype, true, total, heads, head_dim, table, rot_pairs, gamma_q, gamma_k);
  if (st == WCN_SUCCESS && gamma_q && !inv_norm) st = WCN_ERROR_INVALID_PARAMETERS;
  if (st != WCN_SUCCESS) return st == 1 ? WCN_SUCCESS : st;
  const QkPath p = qk_path(total, heads, head_dim, rot_pairs, dtype_bytes(in_dtype), dtype_bytes(out_dtype), qk_all_aligned16(qkv, out));
  return qk_fwd_any(qkv, in_dtype, out, out_dtype, table, gamma_q, gamma_k, inv_norm, p, conjugate ? 1 : 0, (hipStream_t)stream);
}

int wcn_qk_prologue_bwd(const void* dout, int32_t dout_dtype, const void* qkv, int32_t in_dtype, int64_t total, int32_t heads,
                        int32_t head_dim, const float* table, int32_t rot_pairs, const float* gamma_q, const float* gamma_k,
                        const float* inv_norm, void* dqkv, float* dgamma_q, float* dgamma_k, void* workspace,
                        size_t workspace_bytes, wcn_stream_t stream) {
  // dout is what the forward wrote (f16 / bf16), dqkv what it read (in_dtype)
  int st = qk_check(dqkv, in_dtype, dout, dout_dtype, true, total, heads, head_dim, table, rot_pairs, gamma_q, gamma_k);
  const bool norm = gamma_q != nullptr;
  if ((st == WCN_SUCCESS || st == 1) && norm && workspace_bytes < wcn_qk_prologue_workspace_bytes(total, heads, head_dim))
    st = WCN_ERROR_INVALID_PARAMETERS;
  if (st == WCN_SUCCESS && norm &&
      (!qkv || !inv_norm || !dgamma_q || !dgamma_k || !workspace || !aligned_to(qkv, 2 * (size_t)dtype_bytes(in_dtype))))
    st = WCN_ERROR_INVALID_PARAMETERS;
  if (st != WCN_SUCCESS) return st == 1 ? WCN_SUCCESS : st;
  hipStream_t s = (hipStream_t)stream;
  const int sx = dtype_bytes(in_dtype), sg = dtype_bytes(dout_dtype);
  if (!norm) {
    const QkPath p = qk_path(total, heads, head_dim, rot_pairs, sg, sx, qk_all_aligned16(dout, dqkv));
    return qk_fwd_any(dout, dout_dtype, dqkv, in_dtype, table, nullptr, nullptr, nullptr, p, 1, s);
  }
  const QkPath p = qk_path(total, heads, head_dim, rot_pairs, sx, sg, qk_all_aligned16(dout, dqkv, qkv));
  float* partial = (float*)workspace;
  st = with_dtype(in_dtype, [&](auto tx) {
    return with_dtype16(dout_dtype, [&](auto tg) {
      return qk_bwd_t<decltype(tx), decltype(tg)>(dout, qkv, dqkv, table, gamma_q, gamma_k, inv_norm, partial, p, s);
    });
  });
  if (st != WCN_SUCCESS) return st;
  const int hd = heads * head_dim;
  hipLaunchKernelGGL(qk_dgamma_final_kernel, dim3((unsigned)ceil_div(2 * (int64_t)hd, 16)), dim3(256), 0, s,
                     (const float*)partial, p.g.rows, hd, dgamma_q, dgamma_k);
  return launch_status();
}
