// segmented.hip - per-segment statistics and per-segment arithmetic on a ragged batch: rows [N, c] in f32 / f16 / bf16 and
// cu int32 [K + 1] on the device, segment b = rows [cu[b], cu[b + 1]), empty segments allowed, cu never read on the host
// (reference: nn/functional/segmented_arithmetics.py, nn/functional/normalizations.py, which compose these from
// torch_scatter.segment_csr and one element-wise kernel per operator).
//
//   wcn_seg_stats  one read pass over the rows -> two fp32 [K, c] planes
//       MOMENTS  mean, biased variance.  Centred: Welford per lane, Chan merges above it; never E[x^2] - mean^2.
//       RANGE    min, max and the row of the FIRST extremum of each.
//       DOT      sum g, sum g (x - center[b]): what every backward of the segmented norms and arithmetic needs.
//   wcn_seg_apply  one streaming pass: out = x op y[b], the normalisation (x - a[b]) r[b] gamma + beta, and its backward.
//
// The fixed order.  A segment is cut into chunks of kSegChunk rows counted from ITS OWN first row.  One workgroup reduces one
// chunk: L lanes stand side by side on a row (one piece of VEC channels each), the kSegThreads / L row slots share the
// chunk's rows (slot s takes rows s, s + R, ...), and the slots are merged through LDS as a binary tree.  The chunk's
// result goes to a workspace slot; a second launch merges a segment's slots in chunk order (kSegMergeSlices contiguous runs
// of chunks, then the runs in order).  Which rows meet in which order depends on the segment's length and on (c, dtype,
// alignment) alone: a segment's statistics have the same bits whatever else is in the batch and wherever it starts.  No
// float atomics, no zero-filled workspace.  The chunk -> segment map needs no host read: one workgroup scans
// ceil(len / kSegChunk) into cs [K + 1], every chunk workgroup bisects cs, and the surplus workgroups of the
// ceil(rows / kSegChunk) + K launched leave at once.
//
// cu comes from the device unchecked: every span is clamped to [0, rows], every workspace slot to the slots there are.
#include <float.h>

#include <initializer_list>

#include "row_lists.h"

namespace wcn {

constexpr int kSegThreads = 256;      // threads of a workgroup
constexpr int kSegChunk = 256;        // rows of one chunk of a segment = rows of one tile of the apply pass
constexpr int kSegMergeCols = 32;     // second level: columns of a workgroup
constexpr int kSegMergeSlices = 8;    // second level: runs of chunks of a segment

enum SegMode { kSegMoments = WCN_SEG_MOMENTS, kSegRange = WCN_SEG_RANGE, kSegDot = WCN_SEG_DOT };
enum SegKind { kSegArith = 0, kSegNorm = 1, kSegNormBwd = 2 };

struct SegGeom {
  int64_t rows;
  int64_t cap;     // chunk slots of the workspace: ceil(rows / kSegChunk) + K
  int channels, num_segs;
  int pieces;      // channels / VEC
  int llog;        // L = 1 << llog lanes side by side on a row
};

__host__ __device__ constexpr int seg_planes(int mode) { return mode == kSegRange ? 4 : 2; }

// rows [lo, hi) of segment k, inside [0, rows] whatever cu holds
__device__ __forceinline__ void seg_span(const int32_t* __restrict__ cu, int k, int64_t rows, int64_t& lo, int64_t& hi) {
  lo = cu[k];
  hi = cu[k + 1];
  lo = lo < 0 ? 0 : lo > rows ? rows : lo;
  hi = hi < lo ? lo : hi > rows ? rows : hi;
}

// ---- merges ---------------------------------------------------------------------------------------------------------------
// (na, mean a, M2 a) <- merged with (nb, mean b, M2 b), Chan et al.; the counts travel beside the call
__device__ __forceinline__ void chan_merge(float na, float& ma, float& qa, float nb, float mb, float qb) {
  if (nb <= 0.f) return;
  if (na <= 0.f) { ma = mb; qa = qb; return; }
  const float d = mb - ma, f = nb / (na + nb);
  ma += d * f;
  qa += qb + d * d * (na * f);
}

// the smaller (LESS) or larger value; of two equal ones the smaller row.  INT_MAX = no row yet.
template <bool LESS>
__device__ __forceinline__ void ext_merge(float& va, int& ia, float vb, int ib) {
  if (ib == INT_MAX) return;
  const bool better = LESS ? vb < va : vb > va;
  if (ia == INT_MAX || better || (vb == va && ib < ia)) { va = vb; ia = ib; }
}

// rows i < len with i = s (mod stride)
__device__ __forceinline__ int slot_rows(int s, int stride, int len) { return s < len ? (len - s + stride - 1) / stride : 0; }

// ---- the plan: cs[k] = first chunk slot of segment k, cs[K] = chunks in all.  ONE workgroup. ---------------------------------
__global__ __launch_bounds__(kSegThreads) void seg_plan_kernel(const int32_t* __restrict__ cu, int K, int64_t rows, int64_t cap,
                                                               int32_t* __restrict__ cs) {
  __shared__ int s_wave[kSegThreads / 64];
  int64_t carry = 0;
  for (int64_t base = 0; base < K; base += kSegThreads) {
    const int64_t i = base + threadIdx.x;
    int v = 0;
    if (i < K) {
      int64_t lo, hi;
      seg_span(cu, (int)i, rows, lo, hi);
      v = (int)((hi - lo + kSegChunk - 1) / kSegChunk);
    }
    int tot;
    const int e = block_excl_scan<kSegThreads>(v, s_wave, &tot);
    if (i < K) {
      const int64_t at = carry + e;
      cs[i] = (int32_t)(at < cap ? at : cap);
    }
    carry += tot;
    __syncthreads();  // s_wave is rewritten by the next trip
  }
  if (threadIdx.x == 0) cs[K] = (int32_t)(carry < cap ? carry : cap);
}

// ---- first level: one workgroup per chunk ----------------------------------------------------------------------------------
// part [cap][planes][c]: MOMENTS (mean, M2), DOT (sum g, sum g (x - center)), RANGE (min, max, row of min, row of max as int)
template <typename T, int VEC, int MODE>
__global__ __launch_bounds__(kSegThreads) void seg_chunk_kernel(const T* __restrict__ x, const T* __restrict__ g,
                                                                const float* __restrict__ center,
                                                                const int32_t* __restrict__ cu, const int32_t* __restrict__ cs,
                                                                float* __restrict__ part, const SegGeom q) {
  constexpr int PL = seg_planes(MODE);
  constexpr bool RANGE = MODE == kSegRange;
  __shared__ float s_a[VEC][kSegThreads], s_b[VEC][kSegThreads];
  __shared__ int s_i[RANGE ? VEC : 1][kSegThreads], s_j[RANGE ? VEC : 1][kSegThreads];

  const int L = 1 << q.llog, R = kSegThreads >> q.llog;
  const int tid = threadIdx.x, cl = tid & (L - 1), rs = tid >> q.llog;
  const int piece = blockIdx.y * L + cl;
  const bool col_ok = piece < q.pieces;
  const int c0 = piece * VEC, C = q.channels, K = q.num_segs;
  const bool has_x = x != nullptr, has_center = center != nullptr;

  int64_t total = cs[K];
  if (total > q.cap) total = q.cap;
  for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const int k = last_offset_not_above(cs, K, w);
    int64_t lo, hi;
    seg_span(cu, k, q.rows, lo, hi);
    const int64_t j = w - cs[k];
    const int64_t r0 = lo + j * kSegChunk;
    const int len = j >= 0 && r0 < hi ? (int)(hi - r0 < kSegChunk ? hi - r0 : kSegChunk) : 0;

    float a[VEC], b[VEC];
    int ia[RANGE ? VEC : 1], ib[RANGE ? VEC : 1];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      a[e] = 0.f;
      b[e] = 0.f;
      if constexpr (RANGE) { ia[e] = INT_MAX; ib[e] = INT_MAX; }
    }
    if (col_ok) {
      float ctr[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) ctr[e] = 0.f;
      if constexpr (MODE == kSegDot) {
        if (has_center) ld_vec<float, VEC>(center + (int64_t)k * C + c0, ctr);
      }
      float n = 0.f;
      for (int i = rs; i < len; i += R) {
        const int64_t row = r0 + i;
        const int64_t at = row * C + c0;
        float v[VEC];
        if constexpr (MODE == kSegMoments) {
          ld_vec<T, VEC>(x + at, v);
          n += 1.f;
          const float inv = 1.f / n;
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const float d = v[e] - a[e];
            a[e] += d * inv;
            b[e] += d * (v[e] - a[e]);
          }
        } else if constexpr (RANGE) {
          ld_vec<T, VEC>(x + at, v);
          const bool first = i == rs;  // the slot's first row is taken as it is
#pragma unroll
          for (int e = 0; e < VEC; ++e) {  // rows ascend: a strict comparison keeps the first
            if (first || v[e] < a[e]) { a[e] = v[e]; ia[e] = (int)row; }
            if (first || v[e] > b[e]) { b[e] = v[e]; ib[e] = (int)row; }
          }
        } else {
          ld_vec<T, VEC>(g + at, v);
#pragma unroll
          for (int e = 0; e < VEC; ++e) a[e] += v[e];
          if (has_x) {
            float xv[VEC];
            ld_vec<T, VEC>(x + at, xv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) b[e] += v[e] * (xv[e] - ctr[e]);
          }
        }
      }
    }

    // the R row slots of a lane column, a binary tree in a fixed order: slot s takes slot s + stride
    if (R > 1) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        s_a[e][tid] = a[e];
        s_b[e][tid] = b[e];
        if constexpr (RANGE) { s_i[e][tid] = ia[e]; s_j[e][tid] = ib[e]; }
      }
      __syncthreads();
      for (int s = R >> 1; s >= 1; s >>= 1) {
        if (rs < s) {
          const int o = tid + (s << q.llog);
          const float na = (float)slot_rows(rs, 2 * s, len), nb = (float)slot_rows(rs + s, 2 * s, len);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            if constexpr (MODE == kSegMoments) {
              chan_merge(na, a[e], b[e], nb, s_a[e][o], s_b[e][o]);
            } else if constexpr (RANGE) {
              ext_merge<true>(a[e], ia[e], s_a[e][o], s_i[e][o]);
              ext_merge<false>(b[e], ib[e], s_b[e][o], s_j[e][o]);
            } else {
              a[e] += s_a[e][o];
              b[e] += s_b[e][o];
            }
            s_a[e][tid] = a[e];
            s_b[e][tid] = b[e];
            if constexpr (RANGE) { s_i[e][tid] = ia[e]; s_j[e][tid] = ib[e]; }
          }
        }
        __syncthreads();
      }
    }
    if (rs == 0 && col_ok) {
      float* p = part + (w * PL) * (int64_t)C + c0;
      st_vec<float, VEC>(p, a);
      st_vec<float, VEC>(p + C, b);
      if constexpr (RANGE) {
        float fa[VEC], fb[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) { fa[e] = __int_as_float(ia[e]); fb[e] = __int_as_float(ib[e]); }
        st_vec<float, VEC>(p + 2 * (int64_t)C, fa);
        st_vec<float, VEC>(p + 3 * (int64_t)C, fb);
      }
    }
  }
}

// ---- second level: a segment's chunk slots in chunk order ------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(kSegMergeCols* kSegMergeSlices) void seg_merge_kernel(
    const float* __restrict__ part, const int32_t* __restrict__ cu, const int32_t* __restrict__ cs, const SegGeom q,
    float* __restrict__ out0, float* __restrict__ out1, int64_t* __restrict__ arg0, int64_t* __restrict__ arg1) {
  constexpr int PL = seg_planes(MODE);
  constexpr bool RANGE = MODE == kSegRange;
  __shared__ float s_a[kSegMergeSlices][kSegMergeCols + 1], s_b[kSegMergeSlices][kSegMergeCols + 1];
  __shared__ int s_i[RANGE ? kSegMergeSlices : 1][kSegMergeCols + 1], s_j[RANGE ? kSegMergeSlices : 1][kSegMergeCols + 1];
  const int cl = threadIdx.x % kSegMergeCols, sl = threadIdx.x / kSegMergeCols;
  const int col = blockIdx.y * kSegMergeCols + cl;
  const int C = q.channels;

  for (int64_t k = blockIdx.x; k < q.num_segs; k += gridDim.x) {
    int64_t lo, hi;
    seg_span(cu, (int)k, q.rows, lo, hi);
    const int64_t len = hi - lo;
    const int64_t nch = (len + kSegChunk - 1) / kSegChunk;
    const int64_t first = cs[k];
    const int64_t per = (nch + kSegMergeSlices - 1) / kSegMergeSlices;
    // rows of the chunks [j0, j1)
    auto run_rows = [&](int64_t j0, int64_t j1) {
      const int64_t r0 = j0 * kSegChunk, r1 = j1 * kSegChunk < len ? j1 * kSegChunk : len;
      return r1 > r0 ? (float)(r1 - r0) : 0.f;
    };
    const int64_t j0 = sl * per < nch ? sl * per : nch, j1 = j0 + per < nch ? j0 + per : nch;

    float a = 0.f, b = 0.f, n = 0.f;
    int ia = INT_MAX, ib = INT_MAX;
    if (col < C) {
      for (int64_t j = j0; j < j1; ++j) {
        const int64_t slot = first + j;
        if (slot < 0 || slot >= q.cap) continue;
        const float* p = part + (slot * PL) * (int64_t)C + col;
        const float pa = p[0], pb = p[C];
        const float nj = run_rows(j, j + 1);
        if constexpr (MODE == kSegMoments) {
          chan_merge(n, a, b, nj, pa, pb);
          n += nj;
        } else if constexpr (RANGE) {
          ext_merge<true>(a, ia, pa, __float_as_int(p[2 * (int64_t)C]));
          ext_merge<false>(b, ib, pb, __float_as_int(p[3 * (int64_t)C]));
        } else {
          a += pa;
          b += pb;
        }
      }
    }
    s_a[sl][cl] = a;
    s_b[sl][cl] = b;
    if constexpr (RANGE) { s_i[sl][cl] = ia; s_j[sl][cl] = ib; }
    __syncthreads();
    if (sl == 0 && col < C) {
      float na = run_rows(0, per < nch ? per : nch);
#pragma unroll
      for (int s = 1; s < kSegMergeSlices; ++s) {
        const int64_t t0 = s * per < nch ? s * per : nch, t1 = t0 + per < nch ? t0 + per : nch;
        const float nb = run_rows(t0, t1);
        if constexpr (MODE == kSegMoments) {
          chan_merge(na, a, b, nb, s_a[s][cl], s_b[s][cl]);
          na += nb;
        } else if constexpr (RANGE) {
          ext_merge<true>(a, ia, s_a[s][cl], s_i[s][cl]);
          ext_merge<false>(b, ib, s_b[s][cl], s_j[s][cl]);
        } else {
          a += s_a[s][cl];
          b += s_b[s][cl];
        }
      }
      const int64_t at = k * C + col;
      if constexpr (MODE == kSegMoments) {
        out0[at] = len > 0 ? a : 0.f;
        out1[at] = len > 0 ? b / (float)len : 0.f;
      } else if constexpr (RANGE) {  // an empty segment: 0 and -1
        out0[at] = ia == INT_MAX ? 0.f : a;
        out1[at] = ib == INT_MAX ? 0.f : b;
        if (arg0) arg0[at] = ia == INT_MAX ? -1 : (int64_t)ia;
        if (arg1) arg1[at] = ib == INT_MAX ? -1 : (int64_t)ib;
      } else {
        out0[at] = a;
        if (out1) out1[at] = b;
      }
    }
    __syncthreads();  // the LDS planes are rewritten by the next trip
  }
}

// ---- the streaming pass ----------------------------------------------------------------------------------------------------
struct SegApplyArgs {
  const void* x;
  const void* g;
  const void* y;
  const float* a;
  const float* r;
  const float* gamma;
  const float* beta;
  const float* s0;
  const float* s1;
  const int32_t* cu;
  void* out;
  int op;
};

// One workgroup per tile of kSegChunk rows: it bisects cu for the segment of the tile's first row, and every lane walks on
// from there over its rows (row slot s takes rows s, s + R, ...), reading a segment's [K, c] values when the segment changes.
template <typename T, typename Y, int VEC, int KIND>
__global__ __launch_bounds__(kSegThreads) void seg_apply_kernel(const SegApplyArgs p, const SegGeom q) {
  const T* __restrict__ x = (const T*)p.x;
  const T* __restrict__ g = (const T*)p.g;
  const Y* __restrict__ y = (const Y*)p.y;
  T* __restrict__ out = (T*)p.out;
  const int32_t* __restrict__ cu = p.cu;
  const int L = 1 << q.llog, R = kSegThreads >> q.llog;
  const int cl = threadIdx.x & (L - 1), rs = threadIdx.x >> q.llog;
  const int C = q.channels, K = q.num_segs;
  const int64_t ntiles = (q.rows + kSegChunk - 1) / kSegChunk;

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t t0 = tile * kSegChunk;
    const int64_t t1 = t0 + kSegChunk < q.rows ? t0 + kSegChunk : q.rows;
    const int b0 = last_offset_not_above(cu, K, t0);
    for (int piece = cl; piece < q.pieces; piece += L) {
      const int c0 = piece * VEC;
      float gm[VEC], bt[VEC], u[VEC], v[VEC];  // u, v: the segment's values (y | a, r | a, r); gm, bt per channel
#pragma unroll
      for (int e = 0; e < VEC; ++e) { gm[e] = 1.f; bt[e] = 0.f; u[e] = 0.f; v[e] = 0.f; }
      float m0[KIND == kSegNormBwd ? VEC : 1], m1[KIND == kSegNormBwd ? VEC : 1];
      if constexpr (KIND != kSegArith) {
        if (p.gamma) ld_vec<float, VEC>(p.gamma + c0, gm);
        if (p.beta) ld_vec<float, VEC>(p.beta + c0, bt);
      }
      int b = b0;
      int64_t next = b + 1 < K ? (int64_t)cu[b + 1] : LLONG_MAX;
      bool fresh = true;
      for (int64_t t = t0 + rs; t < t1; t += R) {
        while (t >= next) {  // ends at the last segment at the latest
          ++b;
          next = b + 1 < K ? (int64_t)cu[b + 1] : LLONG_MAX;
          fresh = true;
        }
        if (fresh) {
          fresh = false;
          const int64_t at = (int64_t)b * C + c0;
          if constexpr (KIND == kSegArith) {
            ld_vec<Y, VEC>(y + at, u);
          } else {
            if (p.a) ld_vec<float, VEC>(p.a + at, u);
            ld_vec<float, VEC>(p.r + at, v);
          }
          if constexpr (KIND == kSegNormBwd) {
            int64_t lo, hi;
            seg_span(cu, b, q.rows, lo, hi);
            const float inv_n = 1.f / (float)(hi - lo > 1 ? hi - lo : 1);
            ld_vec<float, VEC>(p.s0 + at, m0);
            ld_vec<float, VEC>(p.s1 + at, m1);
#pragma unroll
            for (int e = 0; e < VEC; ++e) { m0[e] *= inv_n; m1[e] *= inv_n; }
          }
        }
        const int64_t at = t * C + c0;
        float xv[VEC], o[VEC];
        ld_vec<T, VEC>(x + at, xv);
        if constexpr (KIND == kSegArith) {
#pragma unroll
          for (int e = 0; e < VEC; ++e)
            o[e] = p.op == WCN_SEG_ADD ? xv[e] + u[e] : p.op == WCN_SEG_SUB ? xv[e] - u[e] : p.op == WCN_SEG_MUL ? xv[e] * u[e]
                                                                                                               : xv[e] / u[e];
        } else if constexpr (KIND == kSegNorm) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) o[e] = ((xv[e] - u[e]) * v[e]) * gm[e] + bt[e];
        } else {
          float gv[VEC];
          ld_vec<T, VEC>(g + at, gv);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            // No contraction here: g gamma is rounded on its own, as it was inside s0.  In a one-row segment (r = 1 /
            // sqrt(eps)) it then meets the very same product in s0 / n and cancels to zero; fused into the subtraction
            // it leaves the product's rounding, below an ulp, times r (measured: 3.6e-5 where the answer is 0).
#pragma clang fp contract(off)
            const float gg = gv[e] * gm[e];
            const float xhat = (xv[e] - u[e]) * v[e];
            o[e] = v[e] * ((gg - m0[e]) - xhat * m1[e]);
          }
        }
        st_vec<T, VEC>(out + at, o);
      }
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static SegGeom seg_geom(int64_t rows, int64_t num_segs, int channels, int vec) {
  SegGeom q;
  q.rows = rows;
  q.cap = ceil_div(rows, kSegChunk) + num_segs;
  q.channels = channels;
  q.num_segs = (int)num_segs;
  q.pieces = channels / vec;
  q.llog = 0;
  while ((1 << q.llog) < q.pieces && (1 << q.llog) < kSegThreads) ++q.llog;
  return q;
}

// elements of a 16-B piece, or 1 where the width or a pointer does not allow one (null = absent, allows)
static int seg_vec(int dtype, int channels, std::initializer_list<const void*> ptrs) {
  const int vec = dtype == WCN_F32 ? 4 : 8;
  if (channels % vec != 0) return 1;
  for (const void* p : ptrs)
    if (!aligned_to(p, 16)) return 1;
  return vec;
}

static size_t seg_plan_bytes(int64_t num_segs) { return align256((size_t)(num_segs + 1) * sizeof(int32_t)); }

// sizes shared by both entries.  WCN_SUCCESS, an error, or 1 = valid but nothing to launch.
static int seg_check(int64_t rows, int64_t num_segs, int32_t channels, int32_t dtype) {
  if (rows < 0 || num_segs < 0 || channels < 1) return WCN_ERROR_INVALID_PARAMETERS;
  if (rows > INT32_MAX || num_segs > INT32_MAX - ceil_div(rows, kSegChunk)) return WCN_ERROR_INVALID_PARAMETERS;  // int32 slots
  if (!dtype_ok(dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  return rows == 0 || num_segs == 0 ? 1 : WCN_SUCCESS;
}

template <typename T, int VEC>
static void seg_stats_launch(int mode, const void* x, const void* g, const float* center, const int32_t* cu, const int32_t* cs,
                             float* part, const SegGeom& q, hipStream_t s) {
  const dim3 grid(capped_grid(q.cap), (unsigned)ceil_div(q.pieces, 1 << q.llog));
  if (mode == kSegMoments)
    hipLaunchKernelGGL((seg_chunk_kernel<T, VEC, kSegMoments>), grid, dim3(kSegThreads), 0, s, (const T*)x, (const T*)g, center,
                       cu, cs, part, q);
  else if (mode == kSegRange)
    hipLaunchKernelGGL((seg_chunk_kernel<T, VEC, kSegRange>), grid, dim3(kSegThreads), 0, s, (const T*)x, (const T*)g, center,
                       cu, cs, part, q);
  else
    hipLaunchKernelGGL((seg_chunk_kernel<T, VEC, kSegDot>), grid, dim3(kSegThreads), 0, s, (const T*)x, (const T*)g, center, cu,
                       cs, part, q);
}

template <typename T, typename Y, int VEC>
static void seg_apply_launch(int kind, const SegApplyArgs& a, const SegGeom& q, hipStream_t s) {
  const dim3 grid(capped_grid(ceil_div(q.rows, kSegChunk)));
  if (kind == kSegArith)
    hipLaunchKernelGGL((seg_apply_kernel<T, Y, VEC, kSegArith>), grid, dim3(kSegThreads), 0, s, a, q);
  else if (kind == kSegNorm)
    hipLaunchKernelGGL((seg_apply_kernel<T, T, VEC, kSegNorm>), grid, dim3(kSegThreads), 0, s, a, q);
  else
    hipLaunchKernelGGL((seg_apply_kernel<T, T, VEC, kSegNormBwd>), grid, dim3(kSegThreads), 0, s, a, q);
}

template <typename T, int VEC>
static void seg_apply_y(int kind, bool y_f32, const SegApplyArgs& a, const SegGeom& q, hipStream_t s) {
  if (y_f32) seg_apply_launch<T, float, VEC>(kind, a, q, s);
  else seg_apply_launch<T, T, VEC>(kind, a, q, s);
}

}  // namespace wcn

using namespace wcn;

int32_t wcn_seg_chunk_rows(void) { return kSegChunk; }
int32_t wcn_seg_max_grid(void) { return kRowMaxGrid; }

size_t wcn_seg_stats_workspace_bytes(int64_t rows, int64_t num_segs, int32_t channels, int32_t mode) {
  if (rows <= 0 || num_segs <= 0 || channels < 1 || mode < WCN_SEG_MOMENTS || mode > WCN_SEG_DOT) return 0;
  return seg_plan_bytes(num_segs) +
         (size_t)(ceil_div(rows, kSegChunk) + num_segs) * seg_planes(mode) * (size_t)channels * sizeof(float);
}

int wcn_seg_stats(int32_t mode, const void* x, const void* g, const float* center, const int32_t* cu, int64_t num_segs,
                  int64_t rows, int32_t channels, int32_t dtype, float* out0, float* out1, int64_t* arg0, int64_t* arg1,
                  void* workspace, size_t workspace_bytes, wcn_stream_t stream) {
  if (mode < WCN_SEG_MOMENTS || mode > WCN_SEG_DOT) return WCN_ERROR_INVALID_PARAMETERS;
  int st = seg_check(rows, num_segs, channels, dtype);
  if (st != WCN_SUCCESS && st != 1) return st;
  const bool dot = mode == WCN_SEG_DOT;
  const bool need_out1 = !dot || x != nullptr;
  if (num_segs > 0 && (!out0 || (need_out1 && !out1))) return WCN_ERROR_INVALID_PARAMETERS;
  if (!aligned_to(out0, 4) || !aligned_to(out1, 4) || !aligned_to(arg0, 8) || !aligned_to(arg1, 8))
    return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  if (st == 1) {  // no rows: zeros (and no row, -1), without a kernel
    const size_t cells = (size_t)num_segs * (size_t)channels;
    if (cells > 0) {
      if (hipMemsetAsync(out0, 0, cells * sizeof(float), s) != hipSuccess) return WCN_ERROR_KERNEL_EXECUTION;
      if (out1 && hipMemsetAsync(out1, 0, cells * sizeof(float), s) != hipSuccess) return WCN_ERROR_KERNEL_EXECUTION;
      if (mode == WCN_SEG_RANGE) {
        if (arg0 && hipMemsetAsync(arg0, 0xff, cells * sizeof(int64_t), s) != hipSuccess) return WCN_ERROR_KERNEL_EXECUTION;
        if (arg1 && hipMemsetAsync(arg1, 0xff, cells * sizeof(int64_t), s) != hipSuccess) return WCN_ERROR_KERNEL_EXECUTION;
      }
    }
    return WCN_SUCCESS;
  }
  if (!cu || !workspace || (dot ? !g : !x)) return WCN_ERROR_INVALID_PARAMETERS;
  if (!aligned_to(cu, 4) || !aligned_to(workspace, 16) || !aligned_to(center, 4) ||
      workspace_bytes < wcn_seg_stats_workspace_bytes(rows, num_segs, channels, mode))
    return WCN_ERROR_INVALID_PARAMETERS;
  const size_t el = dtype_bytes(dtype);
  if (!aligned_to(x, el) || !aligned_to(g, el)) return WCN_ERROR_INVALID_PARAMETERS;

  const int vec = seg_vec(dtype, channels, {x, g, center});
  const SegGeom q = seg_geom(rows, num_segs, channels, vec);
  int32_t* cs = (int32_t*)workspace;
  float* part = (float*)((char*)workspace + seg_plan_bytes(num_segs));
  hipLaunchKernelGGL(seg_plan_kernel, dim3(1), dim3(kSegThreads), 0, s, cu, q.num_segs, rows, q.cap, cs);
  with_dtype_vec<false>(dtype, vec, [&](auto t, auto v) {
    seg_stats_launch<decltype(t), v()>(mode, x, dot ? g : nullptr, dot ? center : nullptr, cu, (const int32_t*)cs, part, q, s);
    return 0;
  });
  const dim3 mgrid(capped_grid(num_segs), (unsigned)ceil_div(channels, kSegMergeCols));
  const dim3 mblock(kSegMergeCols * kSegMergeSlices);
  if (mode == WCN_SEG_MOMENTS)
    hipLaunchKernelGGL(seg_merge_kernel<kSegMoments>, mgrid, mblock, 0, s, (const float*)part, cu, (const int32_t*)cs, q, out0,
                       out1, arg0, arg1);
  else if (mode == WCN_SEG_RANGE)
    hipLaunchKernelGGL(seg_merge_kernel<kSegRange>, mgrid, mblock, 0, s, (const float*)part, cu, (const int32_t*)cs, q, out0,
                       out1, arg0, arg1);
  else
    hipLaunchKernelGGL(seg_merge_kernel<kSegDot>, mgrid, mblock, 0, s, (const float*)part, cu, (const int32_t*)cs, q, out0,
                       need_out1 ? out1 : nullptr, arg0, arg1);
  return launch_status();
}

int wcn_seg_apply(int32_t op, const void* x, const void* g, const void* y, int32_t y_dtype, const float* a, const float* r,
                  const float* gamma, const float* beta, const float* s0, const float* s1, const int32_t* cu, int64_t num_segs,
                  int64_t rows, int32_t channels, int32_t dtype, void* out, wcn_stream_t stream) {
  if (op < WCN_SEG_ADD || op > WCN_SEG_NORM_BWD) return WCN_ERROR_INVALID_PARAMETERS;
  int st = seg_check(rows, num_segs, channels, dtype);
  if (st != WCN_SUCCESS && st != 1) return st;
  const int kind = op <= WCN_SEG_DIV ? kSegArith : op == WCN_SEG_NORM ? kSegNorm : kSegNormBwd;
  if (kind == kSegArith && !dtype_ok(y_dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (kind == kSegArith && y_dtype != dtype && y_dtype != WCN_F32) return WCN_ERROR_INVALID_PARAMETERS;
  if (st == 1) return WCN_SUCCESS;
  if (!x || !cu || !out) return WCN_ERROR_INVALID_PARAMETERS;
  if (kind == kSegArith ? !y : !r) return WCN_ERROR_INVALID_PARAMETERS;
  if (kind == kSegNormBwd && (!g || !s0 || !s1)) return WCN_ERROR_INVALID_PARAMETERS;
  const size_t el = dtype_bytes(dtype);
  if (!aligned_to(x, el) || !aligned_to(g, el) || !aligned_to(out, el) || !aligned_to(y, dtype_bytes(y_dtype)) ||
      !aligned_to(a, 4) || !aligned_to(r, 4) || !aligned_to(gamma, 4) || !aligned_to(beta, 4) || !aligned_to(s0, 4) ||
      !aligned_to(s1, 4) || !aligned_to(cu, 4))
    return WCN_ERROR_INVALID_PARAMETERS;

  SegApplyArgs args;
  args.x = x;
  args.g = kind == kSegNormBwd ? g : nullptr;
  args.y = kind == kSegArith ? y : nullptr;
  args.a = kind == kSegArith ? nullptr : a;
  args.r = kind == kSegArith ? nullptr : r;
  args.gamma = kind == kSegArith ? nullptr : gamma;
  args.beta = kind == kSegNorm ? beta : nullptr;
  args.s0 = kind == kSegNormBwd ? s0 : nullptr;
  args.s1 = kind == kSegNormBwd ? s1 : nullptr;
  args.cu = cu;
  args.out = out;
  args.op = op;
  const bool y_f32 = kind == kSegArith && y_dtype == WCN_F32;
  // a [K, c] plane in the row dtype is read in pieces of the row's width, an fp32 one in 16-B pieces of floats
  const int vec = seg_vec(dtype, channels, {x, args.g, args.y, args.a, args.r, args.gamma, args.beta, args.s0, args.s1, out});
  const SegGeom q = seg_geom(rows, num_segs, channels, vec);
  with_dtype_vec<false>(dtype, vec, [&](auto t, auto v) {
    seg_apply_y<decltype(t), v()>(kind, y_f32, args, q, (hipStream_t)stream);
    return 0;
  });
  return launch_status();
}
