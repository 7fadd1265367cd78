// edgeconv.hip - EdgeConv (DGCNN) without an edge tensor: out[i] = max over the list of i of act(BN(W cat(x_j, x_i) + b)).
// The Linear stands in front of every non-linearity, so the edge pre-activation is z[e = (i <- j)] = P[j] + Q[i] with the
// per-point products P = X_in W_a^T, Q = X_q W_q^T + b (library GEMMs, nn/functional/edge_conv.py).  What is left per edge is
// a gather and an add, and every kernel here recomputes z from P and Q instead of reading an [E, C] tensor:
//
//   wcn_edgeconv_stats            mean / biased variance of z over all E edges (training): sums of (z - p), (z - p)^2 around
//                                 the pivot p = P[nbr[0]] + Q[0], per-workgroup partials, merged in fp64 in workgroup order.
//   wcn_edgeconv_forward          u = a z + s, y = leaky_relu(u), out[i] = the FIRST maximum over the list, arg[i] = its slot.
//   wcn_edgeconv_backward_sums    dbeta = sum g, dgamma = sum g zhat over the M arg-max entries, g = grad_out (u > 0 ? 1 : slope).
//   wcn_edgeconv_backward_query   dQ[i] = sum over the list of i of dz_e, in list order.
//   wcn_edgeconv_backward_input   dP[j] = sum over the incoming edges of j of dz_e, in incoming order (transposed lists:
//                                 perm + offsets); rows of more than kRowChunk incoming edges by the chunk rule of row_lists.h.
//   dz_e = a (t_e - k0 - zhat_e k1), t_e = g at the arg-max edge of (i, c) and 0 elsewhere; k0 = dbeta / E, k1 = dgamma / E in
//   training mode, absent (0) otherwise.
//
// fp32.  Lanes stand along the channels (16-B pieces when C % 4 == 0 and every pointer and row pitch allows, else one
// channel), the row slots of a workgroup take different queries / input rows.  No float atomics; every sum has a fixed order
// that depends on the lists, C and the launch constants alone.  u is formed by the same fused multiply-add everywhere, so the
// backward passes see the sign the forward saw.  Lists come from the device unchecked: spans are clamped to [0, E], a
// neighbour outside [0, N) is skipped, a query outside [0, M) likewise.
#include <algorithm>
#include <initializer_list>

#include "row_lists.h"

namespace wcn {

constexpr int kEcThreads = kRowThreads;
constexpr int kEcBlocks = 256;         // first level of the channel sums: workgroups = partials per channel
constexpr int kEcMaxChannels = 512;
constexpr int kEcInFlight = 4;         // gathered rows requested before the first is used

struct EcLists {
  const float* P;           // [N, .] pitch ld_p
  const float* Q;           // [M, .] pitch ld_q
  const int32_t* nbr;       // [E] rows of P
  const int64_t* splits;    // [M + 1] or null: uniform lists of k
  int64_t E, M, N, ld_p, ld_q;
  int k, C, pieces, llog;   // pieces = C / VEC; 1 << llog lanes side by side on a row
};

struct EcAffine {
  const float* a;      // [C] gamma rstd (1 without BatchNorm)
  const float* s;      // [C] beta - a mu (0 without)
  const float* mu;     // [C] or null
  const float* rstd;   // [C] or null
  const float* k0;     // [C] dbeta / E, or null (eval, no BatchNorm)
  const float* k1;     // [C] dgamma / E, or null
  float slope;
};

__device__ __forceinline__ void ec_span(const EcLists& l, int64_t i, int64_t& e0, int64_t& e1) {
  if (l.splits) {
    e0 = l.splits[i];
    e1 = l.splits[i + 1];
  } else {
    e0 = i * l.k;
    e1 = e0 + l.k;
  }
  e0 = e0 < 0 ? 0 : e0 > l.E ? l.E : e0;
  e1 = e1 < e0 ? e0 : e1 > l.E ? l.E : e1;
}

__device__ __forceinline__ float ec_u(float z, float a, float s) { return __builtin_fmaf(a, z, s); }
__device__ __forceinline__ float ec_act(float u, float slope) { return u > 0.f ? u : slope * u; }
__device__ __forceinline__ float ec_dact(float u, float slope) { return u > 0.f ? 1.f : slope; }

template <int VEC>
__device__ __forceinline__ void ec_ld_opt(const float* __restrict__ p, int c0, float fill, float (&f)[VEC]) {
  if (p) {
    ld_vec<float, VEC>(p + c0, f);
  } else {
#pragma unroll
    for (int v = 0; v < VEC; ++v) f[v] = fill;
  }
}

// the slots of VEC channels: `bytes` (1, 2 or 4) per entry, one access
template <int VEC>
__device__ __forceinline__ void ec_st_arg(void* __restrict__ arg, int bytes, int64_t at, const int (&slot)[VEC]) {
  if (bytes == 1) {
    Vec<int8_t, VEC> v;
#pragma unroll
    for (int e = 0; e < VEC; ++e) v.v[e] = (int8_t)slot[e];
    *reinterpret_cast<Vec<int8_t, VEC>*>((int8_t*)arg + at) = v;
  } else if (bytes == 2) {
    Vec<int16_t, VEC> v;
#pragma unroll
    for (int e = 0; e < VEC; ++e) v.v[e] = (int16_t)slot[e];
    *reinterpret_cast<Vec<int16_t, VEC>*>((int16_t*)arg + at) = v;
  } else {
    Vec<int32_t, VEC> v;
#pragma unroll
    for (int e = 0; e < VEC; ++e) v.v[e] = slot[e];
    *reinterpret_cast<Vec<int32_t, VEC>*>((int32_t*)arg + at) = v;
  }
}
template <int VEC>
__device__ __forceinline__ void ec_ld_arg(const void* __restrict__ arg, int bytes, int64_t at, int (&slot)[VEC]) {
  if (bytes == 1) {
    const Vec<int8_t, VEC> v = *reinterpret_cast<const Vec<int8_t, VEC>*>((const int8_t*)arg + at);
#pragma unroll
    for (int e = 0; e < VEC; ++e) slot[e] = v.v[e];
  } else if (bytes == 2) {
    const Vec<int16_t, VEC> v = *reinterpret_cast<const Vec<int16_t, VEC>*>((const int16_t*)arg + at);
#pragma unroll
    for (int e = 0; e < VEC; ++e) slot[e] = v.v[e];
  } else {
    const Vec<int32_t, VEC> v = *reinterpret_cast<const Vec<int32_t, VEC>*>((const int32_t*)arg + at);
#pragma unroll
    for (int e = 0; e < VEC; ++e) slot[e] = v.v[e];
  }
}

// edges [e0, e1) of one list in order: f(slot, z) for every edge with a neighbour in [0, N); kEcInFlight rows requested at once
template <int VEC, typename F>
__device__ __forceinline__ void ec_walk(const EcLists& l, int64_t e0, int64_t e1, int c0, const float (&q)[VEC], F&& f) {
  int64_t e = e0;
  for (; e + kEcInFlight <= e1; e += kEcInFlight) {
    int j[kEcInFlight];
    float p[kEcInFlight][VEC];
#pragma unroll
    for (int t = 0; t < kEcInFlight; ++t) j[t] = l.nbr[e + t];
#pragma unroll
    for (int t = 0; t < kEcInFlight; ++t) {
      const int64_t jc = j[t] >= 0 && j[t] < l.N ? j[t] : 0;  // (N >= 1: checked on the host)
      ld_vec<float, VEC>(l.P + jc * l.ld_p + c0, p[t]);
    }
#pragma unroll
    for (int t = 0; t < kEcInFlight; ++t) {
      if (j[t] < 0 || j[t] >= l.N) continue;
      float z[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) z[v] = p[t][v] + q[v];
      f((int)(e + t - e0), z);
    }
  }
  for (; e < e1; ++e) {
    const int j = l.nbr[e];
    if (j < 0 || j >= l.N) continue;
    float p[VEC], z[VEC];
    ld_vec<float, VEC>(l.P + (int64_t)j * l.ld_p + c0, p);
#pragma unroll
    for (int v = 0; v < VEC; ++v) z[v] = p[v] + q[v];
    f((int)(e - e0), z);
  }
}

// the pivot of the statistics pass, the same bits wherever it is formed
__device__ __forceinline__ float ec_pivot(const EcLists& l, int c) {
  const int j = l.nbr[0];
  const int64_t jc = j >= 0 && j < l.N ? j : 0;
  return l.P[jc * l.ld_p + c] + l.Q[c];
}

// ---- channel sums: workgroup b owns the queries [b per, (b + 1) per) ---------------------------------------------------------
// MODE 0: d = z - pivot over every edge,              s0 += d,  s1 += d d
// MODE 1: g, zhat at the arg-max edge of every (i, c), s0 += g,  s1 += g zhat
// partial [gridDim.x][2][C]
template <int VEC, int MODE>
__global__ __launch_bounds__(kEcThreads) void ec_sums_kernel(const EcLists l, const EcAffine f, const float* __restrict__ gout,
                                                             const void* __restrict__ arg, int arg_bytes,
                                                             float* __restrict__ partial) {
  __shared__ float s_red[2][kEcThreads * VEC];
  const int L = 1 << l.llog, R = kEcThreads >> l.llog;
  const int tid = threadIdx.x, cl = tid & (L - 1), rs = tid >> l.llog;
  const int64_t per = (l.M + gridDim.x - 1) / gridDim.x;
  const int64_t q0 = (int64_t)blockIdx.x * per, q1 = q0 + per < l.M ? q0 + per : l.M;
  for (int p0 = 0; p0 < l.pieces; p0 += L) {
    const int piece = p0 + cl;
    const bool ok = piece < l.pieces;
    const int c0 = piece * VEC;
    float s0[VEC], s1[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { s0[v] = 0.f; s1[v] = 0.f; }
    if (ok) {
      float pv[VEC], a[VEC], s[VEC], mu[VEC], rstd[VEC];
      if constexpr (MODE == 0) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) pv[v] = ec_pivot(l, c0 + v);
      } else {
        ld_vec<float, VEC>(f.a + c0, a);
        ld_vec<float, VEC>(f.s + c0, s);
        ec_ld_opt<VEC>(f.mu, c0, 0.f, mu);
        ec_ld_opt<VEC>(f.rstd, c0, 1.f, rstd);
      }
      for (int64_t i = q0 + rs; i < q1; i += R) {
        float q[VEC];
        ld_vec<float, VEC>(l.Q + i * l.ld_q + c0, q);
        int64_t e0, e1;
        ec_span(l, i, e0, e1);
        if constexpr (MODE == 0) {
          ec_walk<VEC>(l, e0, e1, c0, q, [&](int, const float(&z)[VEC]) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
              const float d = z[v] - pv[v];
              s0[v] += d;
              s1[v] += d * d;
            }
          });
        } else {
          float go[VEC];
          int slot[VEC];
          ld_vec<float, VEC>(gout + i * l.C + c0, go);
          ec_ld_arg<VEC>(arg, arg_bytes, i * l.C + c0, slot);
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            if (slot[v] < 0 || e0 + slot[v] >= e1) continue;
            const int j = l.nbr[e0 + slot[v]];
            if (j < 0 || j >= l.N) continue;
            const float z = l.P[(int64_t)j * l.ld_p + c0 + v] + q[v];
            const float g = go[v] * ec_dact(ec_u(z, a[v], s[v]), f.slope);
            s0[v] += g;
            s1[v] += g * ((z - mu[v]) * rstd[v]);
          }
        }
      }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) { s_red[0][tid * VEC + v] = s0[v]; s_red[1][tid * VEC + v] = s1[v]; }
    __syncthreads();
    if (rs == 0 && ok) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        float t0 = 0.f, t1 = 0.f;
        for (int r = 0; r < R; ++r) {  // the row slots in slot order
          t0 += s_red[0][((r << l.llog) + cl) * VEC + v];
          t1 += s_red[1][((r << l.llog) + cl) * VEC + v];
        }
        partial[((int64_t)blockIdx.x * 2 + 0) * l.C + c0 + v] = t0;
        partial[((int64_t)blockIdx.x * 2 + 1) * l.C + c0 + v] = t1;
      }
    }
    __syncthreads();  // s_red is rewritten by the next trip
  }
}

// second level: one thread per channel, the workgroups' partials in workgroup order, in fp64
template <int MODE>
__global__ __launch_bounds__(kEcThreads) void ec_sums_final_kernel(const float* __restrict__ partial, int nblocks,
                                                                   const EcLists l, float* __restrict__ out0,
                                                                   float* __restrict__ out1) {
  const int c = blockIdx.x * kEcThreads + threadIdx.x;
  if (c >= l.C) return;
  double t0 = 0.0, t1 = 0.0;
  for (int b = 0; b < nblocks; ++b) {
    t0 += (double)partial[((int64_t)b * 2 + 0) * l.C + c];
    t1 += (double)partial[((int64_t)b * 2 + 1) * l.C + c];
  }
  if constexpr (MODE == 0) {
    const double inv = 1.0 / (double)l.E;
    const double md = t0 * inv;  // mean of z - pivot
    const double var = t1 * inv - md * md;
    out0[c] = (float)((double)ec_pivot(l, c) + md);
    out1[c] = (float)(var > 0.0 ? var : 0.0);
  } else {
    out0[c] = (float)t0;
    out1[c] = (float)t1;
  }
}

// ---- forward: row slot = one query, lanes along the channels --------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(kEcThreads) void ec_forward_kernel(const EcLists l, const EcAffine f, float* __restrict__ out,
                                                                void* __restrict__ arg, int arg_bytes) {
  const int L = 1 << l.llog, R = kEcThreads >> l.llog;
  const int cl = threadIdx.x & (L - 1), rs = threadIdx.x >> l.llog;
  for (int64_t i = (int64_t)blockIdx.x * R + rs; i < l.M; i += (int64_t)gridDim.x * R) {
    int64_t e0, e1;
    ec_span(l, i, e0, e1);
    for (int piece = cl; piece < l.pieces; piece += L) {
      const int c0 = piece * VEC;
      float a[VEC], s[VEC], q[VEC], best[VEC];
      int slot[VEC];
      ld_vec<float, VEC>(f.a + c0, a);
      ld_vec<float, VEC>(f.s + c0, s);
      ld_vec<float, VEC>(l.Q + i * l.ld_q + c0, q);
#pragma unroll
      for (int v = 0; v < VEC; ++v) { best[v] = 0.f; slot[v] = -1; }
      ec_walk<VEC>(l, e0, e1, c0, q, [&](int at, const float(&z)[VEC]) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) {  // slots ascend: a strict comparison keeps the first maximum
          const float y = ec_act(ec_u(z[v], a[v], s[v]), f.slope);
          if (slot[v] < 0 || y > best[v]) { best[v] = y; slot[v] = at; }
        }
      });
      st_vec<float, VEC>(out + i * l.C + c0, best);
      if (arg) ec_st_arg<VEC>(arg, arg_bytes, i * l.C + c0, slot);
    }
  }
}

// dz of one edge and channel
__device__ __forceinline__ float ec_dz(float z, float t, float a, float mu, float rstd, float k0, float k1) {
  return a * ((t - k0) - ((z - mu) * rstd) * k1);
}

// ---- backward by query -----------------------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(kEcThreads) void ec_dq_kernel(const EcLists l, const EcAffine f, const float* __restrict__ gout,
                                                           const void* __restrict__ arg, int arg_bytes,
                                                           float* __restrict__ dq) {
  const int L = 1 << l.llog, R = kEcThreads >> l.llog;
  const int cl = threadIdx.x & (L - 1), rs = threadIdx.x >> l.llog;
  const bool train = f.k0 != nullptr;
  for (int64_t i = (int64_t)blockIdx.x * R + rs; i < l.M; i += (int64_t)gridDim.x * R) {
    int64_t e0, e1;
    ec_span(l, i, e0, e1);
    for (int piece = cl; piece < l.pieces; piece += L) {
      const int c0 = piece * VEC;
      float a[VEC], s[VEC], q[VEC], go[VEC], acc[VEC];
      int slot[VEC];
      ld_vec<float, VEC>(f.a + c0, a);
      ld_vec<float, VEC>(f.s + c0, s);
      ld_vec<float, VEC>(l.Q + i * l.ld_q + c0, q);
      ld_vec<float, VEC>(gout + i * l.C + c0, go);
      ec_ld_arg<VEC>(arg, arg_bytes, i * l.C + c0, slot);
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
      if (train) {
        float mu[VEC], rstd[VEC], k0[VEC], k1[VEC];
        ld_vec<float, VEC>(f.mu + c0, mu);
        ld_vec<float, VEC>(f.rstd + c0, rstd);
        ld_vec<float, VEC>(f.k0 + c0, k0);
        ld_vec<float, VEC>(f.k1 + c0, k1);
        ec_walk<VEC>(l, e0, e1, c0, q, [&](int at, const float(&z)[VEC]) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const float t = at == slot[v] ? go[v] * ec_dact(ec_u(z[v], a[v], s[v]), f.slope) : 0.f;
            acc[v] += ec_dz(z[v], t, a[v], mu[v], rstd[v], k0[v], k1[v]);
          }
        });
      } else {  // dz is non-zero at the arg-max edge alone
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          if (slot[v] < 0 || e0 + slot[v] >= e1) continue;
          const int j = l.nbr[e0 + slot[v]];
          if (j < 0 || j >= l.N) continue;
          const float z = l.P[(int64_t)j * l.ld_p + c0 + v] + q[v];
          acc[v] = a[v] * (go[v] * ec_dact(ec_u(z, a[v], s[v]), f.slope));
        }
      }
      st_vec<float, VEC>(dq + i * l.ld_q + c0, acc);
    }
  }
}

// ---- backward by input point, over the transposed lists ---------------------------------------------------------------------------
struct EcLong : RowList {  // the long rows of the transposed lists and their chunks' partials
  float* part;   // [item_cap][C]
  size_t bytes;
};

static EcLong ec_carve(void* base, int64_t nnz, int64_t c) {
  EcLong w;
  row_list_caps(nnz, w);
  char* p = (char*)base;
  size_t at = 0;
  w.counters = (int32_t*)(p + at);
  at = align256(at + kRowListCounterInts * 4);
  w.item_row = (int32_t*)(p + at);
  at = align256(at + (size_t)w.item_cap * 4);
  w.item_k = (int32_t*)(p + at);
  at = align256(at + (size_t)w.item_cap * 4);
  w.long_row = (int32_t*)(p + at);
  at = align256(at + (size_t)w.long_cap * 4);
  w.long_base = (int32_t*)(p + at);
  at = align256(at + (size_t)w.long_cap * 4);
  w.part = (float*)(p + at);
  at = align256(at + (size_t)w.item_cap * c * 4);
  w.bytes = at;
  return w;
}

struct EcIncoming {
  const int32_t* perm;      // [E] edges sorted by neighbour, ties in ascending edge order
  const int64_t* offsets;   // [N + 1]
  const int32_t* edge_q;    // [E] query of every edge, or null: e / k
};

// ITEMS = false: a whole row of at most kRowChunk incoming edges -> dp; true: one chunk of a long row -> its partial
template <int VEC, bool ITEMS>
__global__ __launch_bounds__(kEcThreads) void ec_dp_kernel(const EcLists l, const EcAffine f, const EcIncoming in,
                                                           const float* __restrict__ gout, const void* __restrict__ arg,
                                                           int arg_bytes, float* __restrict__ dp, EcLong w) {
  const int L = 1 << l.llog, R = kEcThreads >> l.llog;
  const int cl = threadIdx.x & (L - 1), rs = threadIdx.x >> l.llog;
  const bool train = f.k0 != nullptr;
  const int64_t total = ITEMS ? row_list_items(w) : l.N;
  for (int64_t t = (int64_t)blockIdx.x * R + rs; t < total; t += (int64_t)gridDim.x * R) {
    int64_t row = t, j0, j1;
    if (!(ITEMS ? row_list_item(w, t, in.offsets, l.N, l.E, row, j0, j1) : row_span(in.offsets, l.N, l.E, row, j0, j1)))
      continue;
    if (!ITEMS && j1 - j0 > kRowChunk) continue;
    for (int piece = cl; piece < l.pieces; piece += L) {
      const int c0 = piece * VEC;
      float a[VEC], s[VEC], mu[VEC], rstd[VEC], k0[VEC], k1[VEC], p[VEC], acc[VEC];
      ld_vec<float, VEC>(f.a + c0, a);
      ld_vec<float, VEC>(f.s + c0, s);
      ec_ld_opt<VEC>(f.mu, c0, 0.f, mu);
      ec_ld_opt<VEC>(f.rstd, c0, 1.f, rstd);
      ec_ld_opt<VEC>(f.k0, c0, 0.f, k0);
      ec_ld_opt<VEC>(f.k1, c0, 0.f, k1);
      ld_vec<float, VEC>(l.P + row * l.ld_p + c0, p);
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
      for (int64_t jj = j0; jj < j1; ++jj) {
        const int64_t e = in.perm[jj];
        if (e < 0 || e >= l.E) continue;
        const int64_t i = in.edge_q ? (int64_t)in.edge_q[e] : e / l.k;
        if (i < 0 || i >= l.M) continue;
        int64_t e0, e1;
        ec_span(l, i, e0, e1);
        const int at = (int)(e - e0);
        float q[VEC], go[VEC];
        int slot[VEC];
        ld_vec<float, VEC>(l.Q + i * l.ld_q + c0, q);
        ec_ld_arg<VEC>(arg, arg_bytes, i * l.C + c0, slot);
        ld_vec<float, VEC>(gout + i * l.C + c0, go);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const float z = p[v] + q[v];
          const float tv = at == slot[v] ? go[v] * ec_dact(ec_u(z, a[v], s[v]), f.slope) : 0.f;
          if (train) acc[v] += ec_dz(z, tv, a[v], mu[v], rstd[v], k0[v], k1[v]);
          else if (at == slot[v]) acc[v] += a[v] * tv;
        }
      }
      if (ITEMS) {
        st_vec<float, VEC>(w.part + t * l.C + c0, acc);
      } else {
        st_vec<float, VEC>(dp + row * l.ld_p + c0, acc);
      }
    }
  }
}

// a long row's partials in chunk order
template <int = 0>
__global__ __launch_bounds__(kEcThreads) void ec_dp_combine_kernel(const EcLists l, const EcIncoming in, float* __restrict__ dp,
                                                                   EcLong w, int Lc) {
  const int groups = kEcThreads / Lc;
  const int g = threadIdx.x / Lc, sub = threadIdx.x % Lc;
  const int64_t total = row_list_long_rows(w);
  for (int64_t t = (int64_t)blockIdx.x * groups + g; t < total; t += (int64_t)gridDim.x * groups) {
    int64_t row, len, first, nch;
    if (!row_list_long_row(w, t, in.offsets, l.N, row, len, first, nch)) continue;
    for (int c = sub; c < l.C; c += Lc) {
      float acc = w.part[first * l.C + c];
      for (int64_t k = 1; k < nch; ++k) acc += w.part[(first + k) * l.C + c];
      dp[row * l.ld_p + c] = acc;
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static bool ec_vec4(const EcLists& l, std::initializer_list<const void*> ptrs) {
  if (l.C % 4 != 0 || l.ld_p % 4 != 0 || l.ld_q % 4 != 0) return false;
  for (const void* p : ptrs)
    if (!aligned_to(p, 16)) return false;
  return true;
}

static void ec_shape(EcLists& l, int vec) {
  l.pieces = l.C / vec;
  l.llog = 0;
  while ((1 << l.llog) < l.pieces && (1 << l.llog) < 64) ++l.llog;
}

// WCN_SUCCESS, an error, or 1 = valid but nothing to launch (no queries)
static int ec_check(EcLists& l, const float* P, int64_t ld_p, const float* Q, int64_t ld_q, const int32_t* nbr,
                    const int64_t* splits, int32_t k, int64_t E, int64_t M, int64_t N, int32_t C) {
  if (E < 0 || M < 0 || N < 0 || C < 1 || ld_p < C || ld_q < C) return WCN_ERROR_INVALID_PARAMETERS;
  if (C > kEcMaxChannels) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (E > INT32_MAX || M > INT32_MAX || N > INT32_MAX) return WCN_ERROR_INVALID_PARAMETERS;  // int32 rows, edges and slots
  if (!splits && (k < 1 || (int64_t)k * M != E)) return WCN_ERROR_INVALID_PARAMETERS;
  if (!aligned_to(P, 4) || !aligned_to(Q, 4) || !aligned_to(nbr, 4) || !aligned_to(splits, 8))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (M > 0 && !Q) return WCN_ERROR_INVALID_PARAMETERS;
  if (E > 0 && (!P || !nbr || N < 1)) return WCN_ERROR_INVALID_PARAMETERS;
  l.P = P; l.Q = Q; l.nbr = nbr; l.splits = splits;
  l.E = E; l.M = M; l.N = N; l.ld_p = ld_p; l.ld_q = ld_q;
  l.k = splits ? 1 : k;
  l.C = C;
  return M == 0 ? 1 : WCN_SUCCESS;
}

static bool ec_arg_ok(const void* arg, int32_t arg_bytes) {
  return (arg_bytes == 1 || arg_bytes == 2 || arg_bytes == 4) && aligned_to(arg, 16);
}

}  // namespace wcn

using namespace wcn;

int32_t wcn_edgeconv_max_channels(void) { return kEcMaxChannels; }
int32_t wcn_edgeconv_sum_blocks(void) { return kEcBlocks; }

int32_t wcn_edgeconv_arg_bytes(int64_t longest_list) { return longest_list <= 127 ? 1 : longest_list <= 32767 ? 2 : 4; }

size_t wcn_edgeconv_sums_workspace_bytes(int32_t channels) {
  return channels > 0 ? (size_t)kEcBlocks * 2 * (size_t)channels * sizeof(float) : 0;
}

size_t wcn_edgeconv_backward_input_workspace_bytes(int64_t num_edges, int32_t channels) {
  if (num_edges <= 0 || channels < 1) return 0;
  return ec_carve(nullptr, num_edges, channels).bytes;
}

int wcn_edgeconv_stats(const float* P, int64_t ld_p, const float* Q, int64_t ld_q, const int32_t* nbr, const int64_t* row_splits,
                       int32_t k, int64_t num_edges, int64_t num_queries, int64_t num_inputs, int32_t channels, float* mean,
                       float* var, void* workspace, size_t workspace_bytes, wcn_stream_t stream) {
  EcLists l;
  const int st = ec_check(l, P, ld_p, Q, ld_q, nbr, row_splits, k, num_edges, num_queries, num_inputs, channels);
  if (st != WCN_SUCCESS && st != 1) return st;
  if (num_edges < 1) return WCN_ERROR_INVALID_PARAMETERS;  // statistics of nothing
  if (!mean || !var || !workspace || !aligned_to(mean, 4) || !aligned_to(var, 4) || !aligned_to(workspace, 16) ||
      workspace_bytes < wcn_edgeconv_sums_workspace_bytes(channels))
    return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  const int vec = ec_vec4(l, {P, Q}) ? 4 : 1;
  ec_shape(l, vec);
  const int R = kEcThreads >> l.llog;
  const int blocks = (int)std::min<int64_t>(kEcBlocks, ceil_div(l.M, R));
  const EcAffine f{};
  float* partial = (float*)workspace;
  if (vec == 4)
    hipLaunchKernelGGL((ec_sums_kernel<4, 0>), dim3(blocks), dim3(kEcThreads), 0, s, l, f, (const float*)nullptr,
                       (const void*)nullptr, 0, partial);
  else
    hipLaunchKernelGGL((ec_sums_kernel<1, 0>), dim3(blocks), dim3(kEcThreads), 0, s, l, f, (const float*)nullptr,
                       (const void*)nullptr, 0, partial);
  hipLaunchKernelGGL(ec_sums_final_kernel<0>, dim3((unsigned)ceil_div(channels, kEcThreads)), dim3(kEcThreads), 0, s,
                     (const float*)partial, blocks, l, mean, var);
  return launch_status();
}

int wcn_edgeconv_forward(const float* P, int64_t ld_p, const float* Q, int64_t ld_q, const int32_t* nbr, const int64_t* row_splits,
                         int32_t k, int64_t num_edges, int64_t num_queries, int64_t num_inputs, int32_t channels, const float* a,
                         const float* s, float slope, float* out, void* arg, int32_t arg_bytes, wcn_stream_t stream) {
  EcLists l;
  const int st = ec_check(l, P, ld_p, Q, ld_q, nbr, row_splits, k, num_edges, num_queries, num_inputs, channels);
  if (st != WCN_SUCCESS) return st == 1 ? WCN_SUCCESS : st;
  if (!a || !s || !out || !aligned_to(a, 4) || !aligned_to(s, 4) || !aligned_to(out, 4) || (arg && !ec_arg_ok(arg, arg_bytes)))
    return WCN_ERROR_INVALID_PARAMETERS;
  const int vec = ec_vec4(l, {P, Q, a, s, out}) ? 4 : 1;
  ec_shape(l, vec);
  EcAffine f{};
  f.a = a; f.s = s; f.slope = slope;
  const dim3 grid(capped_grid(ceil_div(l.M, kEcThreads >> l.llog)));
  if (vec == 4) hipLaunchKernelGGL(ec_forward_kernel<4>, grid, dim3(kEcThreads), 0, (hipStream_t)stream, l, f, out, arg, arg_bytes);
  else hipLaunchKernelGGL(ec_forward_kernel<1>, grid, dim3(kEcThreads), 0, (hipStream_t)stream, l, f, out, arg, arg_bytes);
  return launch_status();
}

int wcn_edgeconv_backward_sums(const float* P, int64_t ld_p, const float* Q, int64_t ld_q, const int32_t* nbr,
                               const int64_t* row_splits, int32_t k, int64_t num_edges, int64_t num_queries, int64_t num_inputs,
                               int32_t channels, const float* a, const float* s, const float* mu, const float* rstd, float slope,
                               const float* grad_out, const void* arg, int32_t arg_bytes, float* dbeta, float* dgamma,
                               void* workspace, size_t workspace_bytes, wcn_stream_t stream) {
  EcLists l;
  const int st = ec_check(l, P, ld_p, Q, ld_q, nbr, row_splits, k, num_edges, num_queries, num_inputs, channels);
  if (st != WCN_SUCCESS && st != 1) return st;
  if (!dbeta || !dgamma || !aligned_to(dbeta, 4) || !aligned_to(dgamma, 4)) return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t hs = (hipStream_t)stream;
  if (st == 1) {
    if (hipMemsetAsync(dbeta, 0, (size_t)channels * 4, hs) != hipSuccess) return WCN_ERROR_KERNEL_EXECUTION;
    if (hipMemsetAsync(dgamma, 0, (size_t)channels * 4, hs) != hipSuccess) return WCN_ERROR_KERNEL_EXECUTION;
    return WCN_SUCCESS;
  }
  if (!a || !s || !grad_out || !arg || !ec_arg_ok(arg, arg_bytes) || !workspace || !aligned_to(workspace, 16) ||
      !aligned_to(a, 4) || !aligned_to(s, 4) || !aligned_to(mu, 4) || !aligned_to(rstd, 4) || !aligned_to(grad_out, 4) ||
      workspace_bytes < wcn_edgeconv_sums_workspace_bytes(channels))
    return WCN_ERROR_INVALID_PARAMETERS;
  const int vec = ec_vec4(l, {Q, a, s, mu, rstd, grad_out}) ? 4 : 1;
  ec_shape(l, vec);
  const int R = kEcThreads >> l.llog;
  const int blocks = (int)std::min<int64_t>(kEcBlocks, ceil_div(l.M, R));
  EcAffine f{};
  f.a = a; f.s = s; f.mu = mu; f.rstd = rstd; f.slope = slope;
  float* partial = (float*)workspace;
  if (vec == 4)
    hipLaunchKernelGGL((ec_sums_kernel<4, 1>), dim3(blocks), dim3(kEcThreads), 0, hs, l, f, grad_out, arg, arg_bytes, partial);
  else
    hipLaunchKernelGGL((ec_sums_kernel<1, 1>), dim3(blocks), dim3(kEcThreads), 0, hs, l, f, grad_out, arg, arg_bytes, partial);
  hipLaunchKernelGGL(ec_sums_final_kernel<1>, dim3((unsigned)ceil_div(channels, kEcThreads)), dim3(kEcThreads), 0, hs,
                     (const float*)partial, blocks, l, dbeta, dgamma);
  return launch_status();
}

// the coefficient pointers of both gradient passes; k0 / k1 come together with mu / rstd or not at all
static bool ec_affine(EcAffine& f, const float* a, const float* s, const float* mu, const float* rstd, const float* k0,
                      const float* k1, float slope) {
  if (!a || !s || (k0 != nullptr) != (k1 != nullptr) || (k0 && (!mu || !rstd))) return false;
  for (const float* p : {a, s, mu, rstd, k0, k1})
    if (!aligned_to(p, 4)) return false;
  f.a = a; f.s = s; f.mu = mu; f.rstd = rstd; f.k0 = k0; f.k1 = k1; f.slope = slope;
  return true;
}

int wcn_edgeconv_backward_query(const float* P, int64_t ld_p, const float* Q, int64_t ld_q, const int32_t* nbr,
                                const int64_t* row_splits, int32_t k, int64_t num_edges, int64_t num_queries, int64_t num_inputs,
                                int32_t channels, const float* a, const float* s, const float* mu, const float* rstd,
                                const float* k0, const float* k1, float slope, const float* grad_out, const void* arg,
                                int32_t arg_bytes, float* dq, wcn_stream_t stream) {
  EcLists l;
  const int st = ec_check(l, P, ld_p, Q, ld_q, nbr, row_splits, k, num_edges, num_queries, num_inputs, channels);
  if (st != WCN_SUCCESS) return st == 1 ? WCN_SUCCESS : st;
  EcAffine f{};
  if (!ec_affine(f, a, s, mu, rstd, k0, k1, slope) || !grad_out || !arg || !ec_arg_ok(arg, arg_bytes) || !dq ||
      !aligned_to(grad_out, 4) || !aligned_to(dq, 4))
    return WCN_ERROR_INVALID_PARAMETERS;
  const int vec = ec_vec4(l, {P, Q, a, s, mu, rstd, k0, k1, grad_out, dq}) ? 4 : 1;
  ec_shape(l, vec);
  const dim3 grid(capped_grid(ceil_div(l.M, kEcThreads >> l.llog)));
  if (vec == 4)
    hipLaunchKernelGGL(ec_dq_kernel<4>, grid, dim3(kEcThreads), 0, (hipStream_t)stream, l, f, grad_out, arg, arg_bytes, dq);
  else
    hipLaunchKernelGGL(ec_dq_kernel<1>, grid, dim3(kEcThreads), 0, (hipStream_t)stream, l, f, grad_out, arg, arg_bytes, dq);
  return launch_status();
}

template <int VEC>
static void ec_dp_launch(const EcLists& l, const EcAffine& f, const EcIncoming& in, const float* gout, const void* arg,
                         int arg_bytes, float* dp, const EcLong& w, hipStream_t s) {
  const int R = kEcThreads >> l.llog;
  hipLaunchKernelGGL((ec_dp_kernel<VEC, false>), dim3(capped_grid(ceil_div(l.N, R))), dim3(kEcThreads), 0, s, l, f, in, gout, arg,
                     arg_bytes, dp, w);
  hipLaunchKernelGGL(row_list_collect_kernel<>, dim3(capped_grid(ceil_div(l.N, kRowThreads))), dim3(kRowThreads), 0, s,
                     in.offsets, l.N, l.E, (const RowList&)w);
  hipLaunchKernelGGL((ec_dp_kernel<VEC, true>), dim3(capped_grid(ceil_div(w.item_cap, R))), dim3(kEcThreads), 0, s, l, f, in, gout,
                     arg, arg_bytes, dp, w);
  const int Lc = row_lanes(l.C);
  hipLaunchKernelGGL(ec_dp_combine_kernel<>, dim3(capped_grid(ceil_div(w.long_cap, kEcThreads / Lc))), dim3(kEcThreads), 0, s, l,
                     in, dp, w, Lc);
}

int wcn_edgeconv_backward_input(const float* P, int64_t ld_p, const float* Q, int64_t ld_q, const int32_t* nbr,
                                const int64_t* row_splits, int32_t k, int64_t num_edges, int64_t num_queries, int64_t num_inputs,
                                int32_t channels, const int32_t* perm, const int64_t* offsets, const int32_t* edge_query,
                                const float* a, const float* s, const float* mu, const float* rstd, const float* k0,
                                const float* k1, float slope, const float* grad_out, const void* arg, int32_t arg_bytes, float* dp,
                                void* workspace, size_t workspace_bytes, wcn_stream_t stream) {
  EcLists l;
  const int st = ec_check(l, P, ld_p, Q, ld_q, nbr, row_splits, k, num_edges, num_queries, num_inputs, channels);
  if (st != WCN_SUCCESS && st != 1) return st;
  if (num_inputs == 0) return WCN_SUCCESS;
  if (!dp || !P || !aligned_to(dp, 4)) return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t hs = (hipStream_t)stream;
  if (num_edges == 0 || st == 1) {  // no edge: zeros, row by row of the pitch
    if (hipMemset2DAsync(dp, (size_t)ld_p * 4, 0, (size_t)channels * 4, (size_t)num_inputs, hs) != hipSuccess)
      return WCN_ERROR_KERNEL_EXECUTION;
    return WCN_SUCCESS;
  }
  EcAffine f{};
  if (!ec_affine(f, a, s, mu, rstd, k0, k1, slope) || !grad_out || !arg || !ec_arg_ok(arg, arg_bytes) || !perm || !offsets ||
      (row_splits && !edge_query) || !aligned_to(perm, 4) || !aligned_to(offsets, 8) || !aligned_to(edge_query, 4) ||
      !aligned_to(grad_out, 4) || !workspace || !aligned_to(workspace, 256) ||
      workspace_bytes < wcn_edgeconv_backward_input_workspace_bytes(num_edges, channels))
    return WCN_ERROR_INVALID_PARAMETERS;
  const int vec = ec_vec4(l, {P, Q, a, s, mu, rstd, k0, k1, grad_out, dp}) ? 4 : 1;
  ec_shape(l, vec);
  const EcLong w = ec_carve(workspace, num_edges, channels);
  if (hipMemsetAsync(w.counters, 0, kRowListCounterInts * 4, hs) != hipSuccess) return WCN_ERROR_KERNEL_EXECUTION;
  EcIncoming in;
  in.perm = perm;
  in.offsets = offsets;
  in.edge_q = row_splits ? edge_query : nullptr;
  if (vec == 4) ec_dp_launch<4>(l, f, in, grad_out, arg, arg_bytes, dp, w, hs);
  else ec_dp_launch<1>(l, f, in, grad_out, arg, arg_bytes, dp, w, hs);
  return launch_status();
}
