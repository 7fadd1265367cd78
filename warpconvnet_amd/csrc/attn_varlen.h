// attn_varlen.h - what the attention kernel files share (attn_varlen.hip: head sizes 16 / 32 / 64, one wave or four per work
// item; attn_varlen_d128.hip: head size 128, a wave pair per work item): the MFMA fragment types, the work item of a flat id,
// the row / transposed-image / accumulator helpers, the split shares and their partial layouts, the delta, combine and reduce
// kernels (templates over the head size), and the checks of the separate-operand entry points.  See attn_varlen.hip for the
// contract and the tile shapes.
#pragma once
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

constexpr int kAttnTile = 32;       // rows of a query / key block (the MFMA edge)
constexpr int kAttnPitch = 36;      // LDS row pitch of a transposed tile image, elements (8-B aligned reads)
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// Row (within its 32-row half) of accumulator register i of lane half h: (i & 3) + 8 (i >> 2) + 4 h.
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// The work item of a flat id: (sequence, block, head).  The caller skips a block that starts past its side's end.
struct AttnItem {
  int64_t beg_q, beg_k;
  int len_q, len_k, b0, hd;
};
__device__ __forceinline__ void attn_item(int64_t id, int nblk, int heads, const int32_t* __restrict__ cu_q,
                                          const int32_t* __restrict__ cu_k, AttnItem& it, int block_rows = kAttnTile) {
  it.hd = (int)(id % heads);
  const int64_t t = id / heads;
  const int64_t seq = t / nblk;
  it.b0 = (int)(t % nblk) * block_rows;
  it.beg_q = cu_q[seq];
  it.len_q = cu_q[seq + 1] - (int)it.beg_q;
  it.beg_k = cu_k[seq];
  it.len_k = cu_k[seq + 1] - (int)it.beg_k;
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

// Q, K, V of a call as the kernels read them: separate row pointers, two strides (elements), two boundary arrays.
template <typename T>
struct AttnOperands {
  const T *q, *k, *v;
  int64_t q_stride, kv_stride;
  const int32_t *cu_q, *cu_k;
  int heads;
};

// Stores rows of d of this lane's column as fp32 (the partials of a split dK/dV sweep): runs of 4 consecutive d.
template <int D>
__device__ __forceinline__ void store_dcol_f32(float* __restrict__ dst, const a_f32x16* acc, int h) {
#pragma unroll
  for (int mb = 0; mb < (D + 31) / 32; ++mb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = 32 * mb + 8 * g + 4 * h;
      if (d < D)
        *reinterpret_cast<float4*>(dst + d) =
            make_float4(acc[mb][4 * g], acc[mb][4 * g + 1], acc[mb][4 * g + 2], acc[mb][4 * g + 3]);
    }
}

// The keys [beg, end) that split `split` of `splits` sweeps: its contiguous share of the sequence's 32-key blocks, the same
// for the one-wave and the shared kernels.  Trailing shares may be empty (beg == end).
__device__ __forceinline__ void attn_key_share(int len_k, int splits, int split, int& beg, int& end) {
  const int64_t nb = (len_k + kAttnTile - 1) / kAttnTile, per = (nb + splits - 1) / splits;
  const int64_t lo = split * per * kAttnTile, hi = (split + 1) * per * kAttnTile;
  beg = (int)(lo < len_k ? lo : len_k);
  end = (int)(hi < len_k ? hi : len_k);
}

// The partials of a split-key sweep (forward and dQ), all fp32 in the caller's workspace.
//   o  [k_splits, total_q, H, D]   forward: the unnormalised accumulator of a share; dQ: its unscaled dq
//   ml [k_splits, total_q, H, 2]   forward only: the share's running maximum (exp2 domain) and sum; (-inf, 0) when empty
struct AttnKSplit {
  int k_splits;
  int64_t total_q;
  float *o, *ml;
};

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

// dk / dv rows from the partials of a split sweep: splits summed in the order 0 .. q_splits - 1, one thread per 4
// consecutive d of a (key row, slot, head).  Rows outside [cu_k[0], cu_k[num_seqs]) belong to no sequence: not written.
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_dkdv_reduce_kernel(const float* __restrict__ part, const int32_t* __restrict__ cu_k,
                                                               int64_t num_seqs, int64_t total_k, int heads, int q_splits,
                                                               float scale, T* __restrict__ dk_out, T* __restrict__ dv_out,
                                                               int64_t dkv_stride) {
  typedef typename AFrag<T>::half_type half;
  const int64_t n = total_k * 2 * heads * (D / 4), slab = total_k * 2 * heads * D;
  const int64_t first = cu_k[0], last = cu_k[num_seqs];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % (D / 4));
    int64_t t = i / (D / 4);
    const int hd = (int)(t % heads);
    t /= heads;
    const int slot = (int)(t & 1);
    const int64_t row = t >> 1;
    if (row < first || row >= last) continue;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < q_splits; ++j) {
      const float4 x = *reinterpret_cast<const float4*>(part + j * slab + 4 * i);
      acc.x += x.x, acc.y += x.y, acc.z += x.z, acc.w += x.w;
    }
    const float mul = slot ? 1.f : scale;
    half o;
    o[0] = (T)(acc.x * mul), o[1] = (T)(acc.y * mul), o[2] = (T)(acc.z * mul), o[3] = (T)(acc.w * mul);
    *reinterpret_cast<half*>((slot ? dv_out : dk_out) + row * dkv_stride + (int64_t)hd * D + 4 * c) = o;
  }
}

// out, lse from the partials of a split-key forward, one thread per 4 consecutive d of a (query row, head); j runs
// 0 .. k_splits - 1 in that order:  M = max_j m_j,  L = sum_j exp2(m_j - M) l_j,  out = sum_j exp2(m_j - M) o_j / L,
// lse = (M + log2 L) ln 2.  No share saw a key (M = -inf): out = 0, lse = -inf.  Rows outside [cu_q[0], cu_q[num_seqs])
// belong to no sequence: not written.
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_fwd_combine_kernel(const AttnKSplit ks, const int32_t* __restrict__ cu_q,
                                                               int64_t num_seqs, int heads, T* __restrict__ out,
                                                               float* __restrict__ lse) {
  typedef typename AFrag<T>::half_type half;
  const int64_t slab = ks.total_q * heads, n = slab * (D / 4);
  const int64_t first = cu_q[0], last = cu_q[num_seqs];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % (D / 4));
    const int64_t th = i / (D / 4), row = th / heads;
    if (row < first || row >= last) continue;
    float M = -INFINITY;
    for (int j = 0; j < ks.k_splits; ++j) M = fmaxf(M, ks.ml[2 * (j * slab + th)]);
    const bool any = M > -INFINITY;
    float L = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (any)
      for (int j = 0; j < ks.k_splits; ++j) {
        const float2 ml = *reinterpret_cast<const float2*>(ks.ml + 2 * (j * slab + th));
        const float wj = __builtin_amdgcn_exp2f(ml.x - M);  // an empty share: exp2(-inf) = 0 against l = 0, o = 0
        const float4 x = *reinterpret_cast<const float4*>(ks.o + (j * slab + th) * D + 4 * c);
        L += wj * ml.y;
        acc.x += wj * x.x, acc.y += wj * x.y, acc.z += wj * x.z, acc.w += wj * x.w;
      }
    const float inv = any ? 1.f / L : 0.f;
    half o;
    o[0] = (T)(acc.x * inv), o[1] = (T)(acc.y * inv), o[2] = (T)(acc.z * inv), o[3] = (T)(acc.w * inv);
    *reinterpret_cast<half*>(out + th * D + 4 * c) = o;
    if (c == 0) lse[th] = any ? (M + __log2f(L)) * kLn2 : -INFINITY;
  }
}

// dq rows from the partials of a split-key dQ sweep: splits summed in the order 0 .. k_splits - 1, scaled, cast.  The
// walk of attn_dkdv_reduce_kernel over [k_splits, total_q, H, D].
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_dq_reduce_kernel(const AttnKSplit ks, const int32_t* __restrict__ cu_q,
                                                             int64_t num_seqs, int heads, float scale, T* __restrict__ dq_out,
                                                             int64_t dq_stride) {
  typedef typename AFrag<T>::half_type half;
  const int64_t slab = ks.total_q * heads, n = slab * (D / 4);
  const int64_t first = cu_q[0], last = cu_q[num_seqs];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % (D / 4));
    const int64_t th = i / (D / 4), row = th / heads;
    const int hd = (int)(th % heads);
    if (row < first || row >= last) continue;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < ks.k_splits; ++j) {
      const float4 x = *reinterpret_cast<const float4*>(ks.o + (j * slab + th) * D + 4 * c);
      acc.x += x.x, acc.y += x.y, acc.z += x.z, acc.w += x.w;
    }
    half o;
    o[0] = (T)(acc.x * scale), o[1] = (T)(acc.y * scale), o[2] = (T)(acc.z * scale), o[3] = (T)(acc.w * scale);
    *reinterpret_cast<half*>(dq_out + row * dq_stride + (int64_t)hd * D + 4 * c) = o;
  }
}

// One call's operands and sizes, already checked.
struct AttnCall {
  const void *q, *k, *v;
  int64_t q_stride, kv_stride;
  const int32_t *cu_q, *cu_k;
  int64_t num_seqs, total_q, total_k;
  int heads, max_q, max_k;
  float scale;
};

template <typename T>
static AttnOperands<T> attn_operands(const AttnCall& c) {
  return AttnOperands<T>{(const T*)c.q, (const T*)c.k, (const T*)c.v, c.q_stride, c.kv_stride, c.cu_q, c.cu_k, c.heads};
}

// Checks of the separate-operand form (both directions).  Same return convention as attn_check; "nothing to launch" is
// left to the caller, which knows what each direction writes.  `supported`: the caller's predicate of (head_dim, dtype).
static int attn_kv_check(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride, const int32_t* cu_q,
                         const int32_t* cu_k, int64_t num_seqs, int64_t total_q, int64_t total_k, int32_t heads,
                         int32_t head_dim, int32_t max_q, int32_t max_k, float scale, int supported) {
  if (num_seqs < 0 || total_q < 0 || total_k < 0 || heads < 1 || head_dim < 1 || max_q < 0 || max_k < 0 || !(scale == scale))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (num_seqs > 0 && (!cu_q || !cu_k)) return WCN_ERROR_INVALID_PARAMETERS;
  if ((total_q > 0 && !q) || (total_k > 0 && (!k || !v))) return WCN_ERROR_INVALID_PARAMETERS;
  if (total_q > INT32_MAX || total_k > INT32_MAX) return WCN_ERROR_INVALID_PARAMETERS;  // cu_* are int32
  if (!supported) return WCN_ERROR_UNSUPPORTED_CONFIG;
  const int64_t hd = (int64_t)heads * head_dim;
  if (q_stride < hd || kv_stride < hd || (q_stride & 7) || (kv_stride & 7)) return WCN_ERROR_INVALID_PARAMETERS;
  if (!aligned_to(q, 16) || !aligned_to(k, 16) || !aligned_to(v, 16)) return WCN_ERROR_INVALID_PARAMETERS;
  return WCN_SUCCESS;
}

}  // namespace wcn
