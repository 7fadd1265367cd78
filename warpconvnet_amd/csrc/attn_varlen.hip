// attn_varlen.hip - block-diagonal ("varlen") multi-head softmax attention over a packed qkv tensor: the core of the
// reference's PatchAttention (nn/modules/attention.py:496 -> flash_attn.flash_attn_varlen_qkvpacked_func, wrapped at
// nn/functional/flash_attn_utils.py:15-82).  Same contract, minus dropout, causal mask and window:
//   qkv [T, 3, H, D] (slot 0 = Q, 1 = K, 2 = V), cu_seqlens int32 [S + 1]; a token attends to the tokens of its own
//   sequence [cu[s], cu[s+1]) only.  Forward: out [T, H, D] in the input dtype, lse [T, H] fp32 (natural log of
//   sum exp(scale * q.k)).  Backward: dqkv [T, 3, H, D], written in place, deterministic (no float atomics).
//
// Tile shape.  One wave (= one workgroup) owns 32 rows of one (sequence, head); the grid is a flat list of
// (sequence, 32-row block, head) triples, head fastest (the heads of a token row share its cache lines), walked with a
// grid-stride loop so no grid dimension caps the number of sequences; a block that starts past its sequence's end
// exits at once, so the host never reads cu_seqlens.  Every product is one v_mfma_f32_32x32x16_{bf16,f16} chain:
//   forward      S^T = K Q^T (key in the registers, query on the lane: the row max / sum of a query is 15 lane-local
//                ops and one swap with lane ^ 32), P^T in the accumulator is the B operand of O^T += V^T P^T as it
//                stands (guide §3 'An accumulator tile as the next MFMA's operand'); V^T comes from a transposed LDS
//                image of the key tile.  The online softmax runs in the exp2 domain with log2(e) folded into the scale.
//   dK, dV       one wave per (sequence, 32-key block, head) sweeps the query blocks of its sequence: S = Q K^T and
//                dP = dO V^T with the key on the lane, dV^T += dO^T P and dK^T += Q^T dS (Q^T, dO^T from LDS images),
//                P recomputed from the forward's LSE; dK and dV of a key are summed by one wave in a fixed order.
//   dQ           one wave per (sequence, 32-query block, head) sweeps the key blocks: S^T, dP^T as in the forward,
//                dQ^T += K^T dS^T (K^T from an LDS image).
//   delta        rowsum(dO * O) per (token, head) into the caller's fp32 workspace, before the two sweeps.
// D in {16, 32, 64}: D / 16 k-steps per score product, one (D <= 32) or two 32-row halves of d per output product
// (D = 16 computes 16 rows it drops; the bound at that size is the exp and the softmax VALU work, not the MFMA).
#include "wcn_common.h"

namespace wcn {

typedef __attribute__((ext_vector_type(8))) __bf16 a_bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 a_f16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 a_bf16x4;
typedef __attribute__((ext_vector_type(4))) _Float16 a_f16x4;
typedef __attribute__((ext_vector_type(16))) float a_f32x16;

template <typename T> struct AFrag;
template <> struct AFrag<__bf16> {
  typedef a_bf16x8 type;
  typedef a_bf16x4 half_type;
  static __device__ __forceinline__ a_f32x16 mfma(a_bf16x8 a, a_bf16x8 b, a_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct AFrag<_Float16> {
  typedef a_f16x8 type;
  typedef a_f16x4 half_type;
  static __device__ __forceinline__ a_f32x16 mfma(a_f16x8 a, a_f16x8 b, a_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

constexpr int kAttnBlock = 32;      // rows of a query / key block (the MFMA edge)
constexpr int kAttnPitch = 36;      // LDS row pitch of a transposed tile image, elements (8-B aligned reads)
constexpr int64_t kAttnMaxGrid = 1 << 22;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// Row (within its 32-row half) of accumulator register i of lane half h: (i & 3) + 8 (i >> 2) + 4 h.
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// The work item of a flat id: (sequence, block, head); false when the block starts past the sequence's end.
struct AttnItem {
  int64_t beg;
  int len, b0, hd;
};
__device__ __forceinline__ bool attn_item(int64_t id, int nblk, int heads, const int32_t* __restrict__ cu, AttnItem& it) {
  it.hd = (int)(id % heads);
  const int64_t t = id / heads;
  const int64_t seq = t / nblk;
  it.b0 = (int)(t % nblk) * kAttnBlock;
  it.beg = cu[seq];
  it.len = cu[seq + 1] - (int)it.beg;
  return it.b0 < it.len;
}

// 8 consecutive elements d0 .. d0+7 of one head's slice of a row, or zeros when the row is outside the sequence.
template <typename T>
__device__ __forceinline__ typename AFrag<T>::type load8(const T* __restrict__ base, int64_t pitch, int row, int len, int d0) {
  typedef typename AFrag<T>::type frag;
  if (row < len) return *reinterpret_cast<const frag*>(base + (int64_t)row * pitch + d0);
  frag z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = (T)0.f;
  return z;
}

// Transposed LDS image img[d][row] of a 32-row tile [row][d] (rows past the sequence end are zeros).
template <typename T, int D>
__device__ __forceinline__ void stage_transposed(T* __restrict__ img, const T* __restrict__ base, int64_t pitch, int row0,
                                                 int len) {
#pragma unroll
  for (int it = 0; it < D / 16; ++it) {
    const int c = threadIdx.x + 64 * it;
    const int row = c & 31, dch = c >> 5;
    const typename AFrag<T>::type v = load8<T>(base, pitch, row0 + row, len, 8 * dch);
#pragma unroll
    for (int e = 0; e < 8; ++e) img[(8 * dch + e) * kAttnPitch + row] = v[e];
  }
}

// The same image from the row fragments the wave already holds: lane (r, h) has rows r, d 16 s + 8 h .. + 7 in frag s,
// which is chunk (row r, d-chunk h + 2 s) of stage_transposed's walk - no second read of the tile.
template <typename T, int D>
__device__ __forceinline__ void stage_frags(T* __restrict__ img, const typename AFrag<T>::type* f, int r, int h) {
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) img[(16 * s + 8 * h + e) * kAttnPitch + r] = f[s][e];
}

// A operand (rows = d of half mb, k = rows 16 s .. 16 s + 15 of the tile in the permuted order of an accumulator used as
// the B operand) read from a transposed image.
template <typename T>
__device__ __forceinline__ typename AFrag<T>::type read_tr(const T* __restrict__ img, int mb, int s, int r, int h) {
  typedef typename AFrag<T>::half_type half;
  const T* p = img + (32 * mb + r) * kAttnPitch + 16 * s + 4 * h;
  const half lo = *reinterpret_cast<const half*>(p);
  const half hi = *reinterpret_cast<const half*>(p + 8);
  typename AFrag<T>::type f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[j] = lo[j];
    f[j + 4] = hi[j];
  }
  return f;
}

// Registers 8 s .. 8 s + 7 of an accumulator as the B operand of k-step s.
template <typename T>
__device__ __forceinline__ typename AFrag<T>::type acc_frag(const float* v, int s) {
  typename AFrag<T>::type f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (T)v[8 * s + j];
  return f;
}

// Stores rows of d (accumulator registers, scaled) of the output column owned by this lane: runs of 4 consecutive d.
template <typename T, int D>
__device__ __forceinline__ void store_dcol(T* __restrict__ dst, const a_f32x16* acc, float mul, int h) {
  typedef typename AFrag<T>::half_type half;
#pragma unroll
  for (int mb = 0; mb < (D + 31) / 32; ++mb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = 32 * mb + 8 * g + 4 * h;
      if (d < D) {
        half v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (T)(acc[mb][4 * g + e] * mul);
        *reinterpret_cast<half*>(dst + d) = v;
      }
    }
}

// ---- forward --------------------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(64) void attn_fwd_kernel(const T* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                      int64_t items, int nblk, int heads, float c2, T* __restrict__ out,
                                                      float* __restrict__ lse) {
  typedef typename AFrag<T>::type frag;
  constexpr int NS = D / 16, NMB = (D + 31) / 32;
  __shared__ __attribute__((aligned(16))) T vt[NMB * 32 * kAttnPitch];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int64_t pitch = 3LL * heads * D;
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    AttnItem w;
    if (!attn_item(id, nblk, heads, cu, w)) continue;
    const T* q = qkv + w.beg * pitch + (int64_t)w.hd * D;
    const T* k = q + (int64_t)heads * D;
    const T* v = k + (int64_t)heads * D;
    frag qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = load8<T>(q, pitch, w.b0 + r, w.len, 16 * s + 8 * h);
    a_f32x16 acc[NMB];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mb][i] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < w.len; k0 += kAttnBlock) {
      a_f32x16 st;
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) st = AFrag<T>::mfma(load8<T>(k, pitch, k0 + r, w.len, 16 * s + 8 * h), qf[s], st);
      __syncthreads();  // the previous tile's reads of vt are done
      stage_transposed<T, D>(vt, v, pitch, k0, w.len);
      float x[16];
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        x[i] = k0 + acc_row(i, h) < w.len ? st[i] * c2 : -INFINITY;
        mx = fmaxf(mx, x[i]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mn = fmaxf(m, mx);  // finite: key k0 is inside the sequence
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      float ls = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        x[i] = __builtin_amdgcn_exp2f(x[i] - mn);
        ls += x[i];
      }
      ls += __shfl_xor(ls, 32);
      l = l * alpha + ls;
      m = mn;
#pragma unroll
      for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[mb][i] *= alpha;
      __syncthreads();  // vt staged
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const frag pf = acc_frag<T>(x, s);
#pragma unroll
        for (int mb = 0; mb < NMB; ++mb) acc[mb] = AFrag<T>::mfma(read_tr<T>(vt, mb, s, r, h), pf, acc[mb]);
      }
    }
    const int row = w.b0 + r;
    if (row < w.len) {
      const int64_t t = w.beg + row;
      store_dcol<T, D>(out + (t * heads + w.hd) * D, acc, 1.f / l, h);
      if (h == 0) lse[t * heads + w.hd] = (m + __log2f(l)) * kLn2;
    }
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------
// delta[t][h] = sum_d dO[t][h][d] * O[t][h][d], fp32, one thread per (token, head).
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_delta_kernel(const T* __restrict__ dout, const T* __restrict__ out, int64_t rows,
                                                         float* __restrict__ delta) {
  typedef typename AFrag<T>::type frag;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < D / 8; ++c) {
    const frag a = *reinterpret_cast<const frag*>(dout + i * D + 8 * c);
    const frag b = *reinterpret_cast<const frag*>(out + i * D + 8 * c);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc += (float)a[e] * (float)b[e];
  }
  delta[i] = acc;
}

// dK, dV of one (sequence, 32-key block, head).
template <typename T, int D>
__global__ __launch_bounds__(64) void attn_bwd_dkdv_kernel(const T* __restrict__ qkv, const T* __restrict__ dout,
                                                           const float* __restrict__ lse, const float* __restrict__ delta,
                                                           const int32_t* __restrict__ cu, int64_t items, int nblk, int heads,
                                                           float c2, float scale, T* __restrict__ dqkv) {
  typedef typename AFrag<T>::type frag;
  constexpr int NS = D / 16, NMB = (D + 31) / 32;
  __shared__ __attribute__((aligned(16))) T qt[NMB * 32 * kAttnPitch];
  __shared__ __attribute__((aligned(16))) T dot[NMB * 32 * kAttnPitch];
  __shared__ __attribute__((aligned(16))) float s_lse[kAttnBlock];
  __shared__ __attribute__((aligned(16))) float s_del[kAttnBlock];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int64_t pitch = 3LL * heads * D, opitch = (int64_t)heads * D;
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    AttnItem w;
    if (!attn_item(id, nblk, heads, cu, w)) continue;
    const T* q = qkv + w.beg * pitch + (int64_t)w.hd * D;
    const T* k = q + (int64_t)heads * D;
    const T* v = k + (int64_t)heads * D;
    const T* dO = dout + w.beg * opitch + (int64_t)w.hd * D;
    const int key = w.b0 + r;
    frag kf[NS], vf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      kf[s] = load8<T>(k, pitch, key, w.len, 16 * s + 8 * h);
      vf[s] = load8<T>(v, pitch, key, w.len, 16 * s + 8 * h);
    }
    a_f32x16 dk[NMB], dv[NMB];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) dk[mb][i] = dv[mb][i] = 0.f;
    for (int q0 = 0; q0 < w.len; q0 += kAttnBlock) {
      a_f32x16 sc, dp;
      frag qf[NS], df[NS];
#pragma unroll
      for (int i = 0; i < 16; ++i) sc[i] = dp[i] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        qf[s] = load8<T>(q, pitch, q0 + r, w.len, 16 * s + 8 * h);
        df[s] = load8<T>(dO, opitch, q0 + r, w.len, 16 * s + 8 * h);
        sc = AFrag<T>::mfma(qf[s], kf[s], sc);
        dp = AFrag<T>::mfma(df[s], vf[s], dp);
      }
      __syncthreads();  // the previous block's reads of the images are done
      stage_frags<T, D>(qt, qf, r, h);
      stage_frags<T, D>(dot, df, r, h);
      {
        const int qr = q0 + r;
        const bool ok = qr < w.len;
        const int64_t t = w.beg + qr;
        if (h == 0) s_lse[r] = ok ? lse[t * heads + w.hd] * kLog2e : 0.f;
        else s_del[r] = ok ? delta[t * heads + w.hd] : 0.f;
      }
      __syncthreads();
      // Rows of sc / dp are queries, the lane's column is its key.  Query rows past the end carry Q = dO = 0, lse =
      // delta = 0: p = 1, dS = 0, and their dO^T / Q^T columns are zero, so they add nothing.
      float p[16], ds[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 L = *reinterpret_cast<const float4*>(s_lse + 8 * g + 4 * h);
        const float4 E = *reinterpret_cast<const float4*>(s_del + 8 * g + 4 * h);
        const float Lv[4] = {L.x, L.y, L.z, L.w}, Ev[4] = {E.x, E.y, E.z, E.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g + e;
          p[i] = key < w.len ? __builtin_amdgcn_exp2f(sc[i] * c2 - Lv[e]) : 0.f;
          ds[i] = p[i] * (dp[i] - Ev[e]);
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const frag pf = acc_frag<T>(p, s), dsf = acc_frag<T>(ds, s);
#pragma unroll
        for (int mb = 0; mb < NMB; ++mb) {
          dv[mb] = AFrag<T>::mfma(read_tr<T>(dot, mb, s, r, h), pf, dv[mb]);
          dk[mb] = AFrag<T>::mfma(read_tr<T>(qt, mb, s, r, h), dsf, dk[mb]);
        }
      }
    }
    if (key < w.len) {
      T* dst = dqkv + (w.beg + key) * pitch + (int64_t)w.hd * D;
      store_dcol<T, D>(dst + (int64_t)heads * D, dk, scale, h);
      store_dcol<T, D>(dst + 2LL * heads * D, dv, 1.f, h);
    }
  }
}

// dQ of one (sequence, 32-query block, head).
template <typename T, int D>
__global__ __launch_bounds__(64) void attn_bwd_dq_kernel(const T* __restrict__ qkv, const T* __restrict__ dout,
                                                         const float* __restrict__ lse, const float* __restrict__ delta,
                                                         const int32_t* __restrict__ cu, int64_t items, int nblk, int heads,
                                                         float c2, float scale, T* __restrict__ dqkv) {
  typedef typename AFrag<T>::type frag;
  constexpr int NS = D / 16, NMB = (D + 31) / 32;
  __shared__ __attribute__((aligned(16))) T kt[NMB * 32 * kAttnPitch];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int64_t pitch = 3LL * heads * D, opitch = (int64_t)heads * D;
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    AttnItem w;
    if (!attn_item(id, nblk, heads, cu, w)) continue;
    const T* q = qkv + w.beg * pitch + (int64_t)w.hd * D;
    const T* k = q + (int64_t)heads * D;
    const T* v = k + (int64_t)heads * D;
    const T* dO = dout + w.beg * opitch + (int64_t)w.hd * D;
    const int row = w.b0 + r;
    const bool ok = row < w.len;
    frag qf[NS], df[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      qf[s] = load8<T>(q, pitch, row, w.len, 16 * s + 8 * h);
      df[s] = load8<T>(dO, opitch, row, w.len, 16 * s + 8 * h);
    }
    const float L = ok ? lse[(w.beg + row) * heads + w.hd] * kLog2e : 0.f;
    const float E = ok ? delta[(w.beg + row) * heads + w.hd] : 0.f;
    a_f32x16 dq[NMB];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) dq[mb][i] = 0.f;
    for (int k0 = 0; k0 < w.len; k0 += kAttnBlock) {
      a_f32x16 st, dpt;
      frag kf[NS];
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = dpt[i] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        kf[s] = load8<T>(k, pitch, k0 + r, w.len, 16 * s + 8 * h);
        st = AFrag<T>::mfma(kf[s], qf[s], st);
        dpt = AFrag<T>::mfma(load8<T>(v, pitch, k0 + r, w.len, 16 * s + 8 * h), df[s], dpt);
      }
      __syncthreads();
      stage_frags<T, D>(kt, kf, r, h);
      // rows are keys, the lane's column its query; keys past the end get p = 0 (their K, V rows were read as zeros)
      float ds[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = k0 + acc_row(i, h) < w.len ? __builtin_amdgcn_exp2f(st[i] * c2 - L) : 0.f;
        ds[i] = p * (dpt[i] - E);
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const frag dsf = acc_frag<T>(ds, s);
#pragma unroll
        for (int mb = 0; mb < NMB; ++mb) dq[mb] = AFrag<T>::mfma(read_tr<T>(kt, mb, s, r, h), dsf, dq[mb]);
      }
    }
    if (ok) store_dcol<T, D>(dqkv + (w.beg + row) * pitch + (int64_t)w.hd * D, dq, scale, h);
  }
}

template <typename T, int D>
static int attn_fwd_t(const void* qkv, const int32_t* cu, int64_t items, int nblk, int heads, float scale, void* out, float* lse,
                      hipStream_t s) {
  const int64_t grid = items < kAttnMaxGrid ? items : kAttnMaxGrid;
  hipLaunchKernelGGL((attn_fwd_kernel<T, D>), dim3((unsigned)grid), dim3(64), 0, s, (const T*)qkv, cu, items, nblk, heads,
                     scale * kLog2e, (T*)out, lse);
  return hipGetLastError() == hipSuccess ? WCN_SUCCESS : WCN_ERROR_KERNEL_EXECUTION;
}

template <typename T, int D>
static int attn_bwd_t(const void* dout, const void* qkv, const void* out, const float* lse, const int32_t* cu, int64_t items,
                      int nblk, int64_t total, int heads, float scale, void* dqkv, float* delta, hipStream_t s) {
  const int64_t rows = total * heads;
  hipLaunchKernelGGL((attn_delta_kernel<T, D>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, (const T*)dout,
                     (const T*)out, rows, delta);
  const int64_t grid = items < kAttnMaxGrid ? items : kAttnMaxGrid;
  hipLaunchKernelGGL((attn_bwd_dkdv_kernel<T, D>), dim3((unsigned)grid), dim3(64), 0, s, (const T*)qkv, (const T*)dout, lse,
                     (const float*)delta, cu, items, nblk, heads, scale * kLog2e, scale, (T*)dqkv);
  hipLaunchKernelGGL((attn_bwd_dq_kernel<T, D>), dim3((unsigned)grid), dim3(64), 0, s, (const T*)qkv, (const T*)dout, lse,
                     (const float*)delta, cu, items, nblk, heads, scale * kLog2e, scale, (T*)dqkv);
  return hipGetLastError() == hipSuccess ? WCN_SUCCESS : WCN_ERROR_KERNEL_EXECUTION;
}

// Shared argument checks of both directions.  Returns WCN_SUCCESS, an error, or 1 = valid but nothing to launch.
static int attn_check(const void* qkv, const int32_t* cu, int64_t num_seqs, int64_t total, int32_t heads, int32_t head_dim,
                      int32_t max_seqlen, float scale, int32_t dtype) {
  if (num_seqs < 0 || total < 0 || heads < 1 || head_dim < 1 || max_seqlen < 0 || !(scale == scale)) return WCN_ERROR_INVALID_PARAMETERS;
  if (num_seqs > 0 && !cu) return WCN_ERROR_INVALID_PARAMETERS;
  if (total > 0 && !qkv) return WCN_ERROR_INVALID_PARAMETERS;
  if (total > INT32_MAX) return WCN_ERROR_INVALID_PARAMETERS;  // cu_seqlens is int32
  if (!wcn_attn_varlen_supported(head_dim, dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (num_seqs == 0 || total == 0 || max_seqlen == 0) return 1;
  return WCN_SUCCESS;
}

#define WCN_ATTN_DISPATCH(CALL)                              \
  switch (head_dim) {                                        \
    case 16: CALL(16);                                       \
    case 32: CALL(32);                                       \
    default: CALL(64);                                       \
  }

}  // namespace wcn

using namespace wcn;

int wcn_attn_varlen_supported(int32_t head_dim, int32_t dtype) {
  return (head_dim == 16 || head_dim == 32 || head_dim == 64) && (dtype == WCN_F16 || dtype == WCN_BF16) ? 1 : 0;
}

size_t wcn_attn_varlen_workspace_bytes(int64_t total, int32_t heads) {
  if (total < 0 || heads < 0) return 0;
  return (size_t)total * (size_t)heads * sizeof(float);
}

int wcn_attn_varlen_fwd(const void* qkv, const int32_t* cu_seqlens, int64_t num_seqs, int64_t total, int32_t heads,
                        int32_t head_dim, int32_t max_seqlen, float softmax_scale, int32_t dtype, void* out, float* lse,
                        wcn_stream_t stream) {
  int st = attn_check(qkv, cu_seqlens, num_seqs, total, heads, head_dim, max_seqlen, softmax_scale, dtype);
  if (st == WCN_SUCCESS && (!out || !lse)) st = WCN_ERROR_INVALID_PARAMETERS;
  if (st != WCN_SUCCESS) return st == 1 ? WCN_SUCCESS : st;
  const int nblk = (max_seqlen + kAttnBlock - 1) / kAttnBlock;
  const int64_t items = num_seqs * nblk * heads;
  hipStream_t s = (hipStream_t)stream;
#define WCN_ATTN_FWD(DD)                                                                                              \
  return dtype == WCN_BF16 ? attn_fwd_t<__bf16, DD>(qkv, cu_seqlens, items, nblk, heads, softmax_scale, out, lse, s)  \
                           : attn_fwd_t<_Float16, DD>(qkv, cu_seqlens, items, nblk, heads, softmax_scale, out, lse, s);
  WCN_ATTN_DISPATCH(WCN_ATTN_FWD)
#undef WCN_ATTN_FWD
}

int wcn_attn_varlen_bwd(const void* dout, const void* qkv, const void* out, const float* lse, const int32_t* cu_seqlens,
                        int64_t num_seqs, int64_t total, int32_t heads, int32_t head_dim, int32_t max_seqlen,
                        float softmax_scale, int32_t dtype, void* dqkv, void* workspace, size_t workspace_bytes,
                        wcn_stream_t stream) {
  int st = attn_check(qkv, cu_seqlens, num_seqs, total, heads, head_dim, max_seqlen, softmax_scale, dtype);
  if (st == WCN_SUCCESS && (!dout || !out || !lse || !dqkv || !workspace ||
                            workspace_bytes < wcn_attn_varlen_workspace_bytes(total, heads)))
    st = WCN_ERROR_INVALID_PARAMETERS;
  if (st != WCN_SUCCESS) return st == 1 ? WCN_SUCCESS : st;
  const int nblk = (max_seqlen + kAttnBlock - 1) / kAttnBlock;
  const int64_t items = num_seqs * nblk * heads;
  hipStream_t s = (hipStream_t)stream;
  float* delta = (float*)workspace;
#define WCN_ATTN_BWD(DD)                                                                                                 \
  return dtype == WCN_BF16                                                                                               \
             ? attn_bwd_t<__bf16, DD>(dout, qkv, out, lse, cu_seqlens, items, nblk, total, heads, softmax_scale, dqkv,    \
                                      delta, s)                                                                         \
             : attn_bwd_t<_Float16, DD>(dout, qkv, out, lse, cu_seqlens, items, nblk, total, heads, softmax_scale, dqkv, \
                                        delta, s);
  WCN_ATTN_DISPATCH(WCN_ATTN_BWD)
#undef WCN_ATTN_BWD
}
