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
// Operands.  The kernels take Q, K and V as separate row pointers: q rows with stride q_stride, k and v rows with one
// common stride kv_stride (elements), and two boundary arrays: sequence s is queries [cu_q[s], cu_q[s+1]) against keys
// [cu_k[s], cu_k[s+1]) (cross-attention: voxel queries against a context).  The packed entry points pass the three slots
// of one [T, 3, H, D] tensor with q_stride = kv_stride = 3 H D and cu_q = cu_k.  out / dout / lse / delta are contiguous
// [Tq, H, D] / [Tq, H].  An empty side is defined, not NaN: a query with no key gets out = 0, lse = -inf, dq = 0; the
// keys of a sequence with no query get dk = dv = 0.
// Split dK/dV sweep.  With few long query sequences (tens of thousands of voxels against ~1000 context tokens) the dK/dV
// pass has only nblk_k * H waves per sequence, each sweeping every query block.  With q_splits > 1 an item is (sequence,
// key block, split, head): split j sweeps its contiguous share of the query blocks and writes unscaled fp32 partials to
// part [q_splits, total_k, 2, H, D]; attn_dkdv_reduce_kernel sums them in the order 0 .. q_splits - 1, scales, casts.
// Shared-tile variants (WCN_ATTN_SHARED: attn_fwd_shared_kernel, attn_bwd_dq_shared_kernel, attn_bwd_dkdv_shared_kernel).
// The kernels above are one wave per workgroup: every wave streams each 32-row tile of the side it sweeps from global
// memory itself - 8 KB per tile at D = 64 for eight MFMAs.  The shared variants run four waves (256 threads) on one
// (sequence, 128-row block, head): wave w owns rows 32 w .. 32 w + 31, and the WORKGROUP stages each tile of the swept side
// once in LDS - row-major (what load8 returns) and as the transposed image the one-wave kernel builds - so global operand
// traffic per owned row drops 4 x.  Staging is double-buffered: the next tile's loads are issued before the current tile's
// MFMAs and written to the other buffer after them, one barrier per tile.  Each wave then issues exactly the one-wave
// kernel's sequence on its rows (same tile order, MFMA chains, exp2-domain softmax, stores): the operands hold the same
// values wherever they were read from, so every output element carries the same bits (tests/test_gpu_attention_shared.py).
// Loop bounds are uniform over the workgroup (one sequence, one split share); a wave whose block lies past the end of its
// side computes on zero rows, stages, reaches every barrier and stores nothing.
// LDS at D = 64, both buffers: forward K rows 32 x 72 x 2 B + V^T 64 x 36 x 2 B = 9 216 B per buffer, 18 KiB -> 8 workgroups
// (32 waves) per CU by LDS, 3 per SIMD by registers (116 VGPRs); dQ K rows + V rows + K^T = 13 824 B, 27 KiB -> 5 workgroups,
// 2 per SIMD by registers (138 VGPRs); dK/dV Q rows + dO rows + Q^T + dO^T + lse + delta = 18 688 B, 36.5 KiB -> 4
// workgroups, 2 per SIMD by registers (161 VGPRs).  Of the 160 KiB of a CU none of them is bound by LDS.
// Split-key sweep (KSPLIT instantiations of the forward and dQ kernels, one-wave and shared).  The mirror case of the split
// dK/dV sweep: a handful of queries per sequence against 10^4 .. 10^5 keys (a query decoder over a whole scene) gives the
// forward and dQ num_seqs * ceil(Lq / 128) * H work items that each walk thousands of key tiles.  With k_splits = S > 1 an
// item is (sequence, query block, split, head); split j sweeps the 32-key blocks [j per, min((j + 1) per, nb)) of its
// sequence, nb = ceil(len_k / 32), per = ceil(nb / S) (attn_key_share: from cu_k on the device, the same keys under both
// variants, trailing shares possibly empty), with the unsplit tile loop.  The forward writes the share's unnormalised
// accumulator o_j [S, Tq, H, D] and (m_j, l_j) [S, Tq, H, 2] in fp32 - an empty share leaves (-inf, 0) and zeros - and
// attn_fwd_combine_kernel forms M = max_j m_j, L = sum_j exp2(m_j - M) l_j, out = sum_j exp2(m_j - M) o_j / L,
// lse = (M + log2 L) ln 2 with j = 0 .. S - 1 in that order.  dQ writes unscaled fp32 dq_j [S, Tq, H, D] (P comes from the
// final LSE: nothing to renormalise) and attn_dq_reduce_kernel adds them in the same order.  Every partial read was written
// by the launch before it: the workspace's earlier contents never matter, and there is no float atomic.  S = 1 launches the
// KSPLIT = false instantiations, whose loop bounds are the constants they always were.
// Resources of the split instantiations at D = 64 (hipcc -Rpass-analysis=kernel-resource-usage): forward one-wave 111 VGPRs,
// 4.5 KiB LDS, shared 114 VGPRs, 18 KiB - 3 waves per SIMD both, as unsplit; dQ one-wave 126 VGPRs, 4.5 KiB, shared 132
// VGPRs, 27 KiB - 3 per SIMD (the unsplit shared dQ: 138 VGPRs, 2 per SIMD); combine 28 VGPRs, reduce 24, no LDS.  None
// spills; none is bound by LDS.
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

// The work item of a flat id: (sequence, block, head).  The caller skips a block that starts past its side's end.
struct AttnItem {
  int64_t beg_q, beg_k;
  int len_q, len_k, b0, hd;
};
__device__ __forceinline__ void attn_item(int64_t id, int nblk, int heads, const int32_t* __restrict__ cu_q,
                                          const int32_t* __restrict__ cu_k, AttnItem& it, int block_rows = kAttnBlock) {
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
  const int64_t nb = (len_k + kAttnBlock - 1) / kAttnBlock, per = (nb + splits - 1) / splits;
  const int64_t lo = split * per * kAttnBlock, hi = (split + 1) * per * kAttnBlock;
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

// ---- forward --------------------------------------------------------------------------------------------------------
// KSPLIT: item ids are (sequence, query block, split, head); the wave sweeps its share of the keys and writes partials.
template <typename T, int D, bool KSPLIT>
__global__ __launch_bounds__(64) void attn_fwd_kernel(const AttnOperands<T> a, int64_t items, int nblk, float c2,
                                                      T* __restrict__ out, float* __restrict__ lse, const AttnKSplit ks) {
  typedef typename AFrag<T>::type frag;
  constexpr int NS = D / 16, NMB = (D + 31) / 32;
  __shared__ __attribute__((aligned(16))) T vt[NMB * 32 * kAttnPitch];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int heads = a.heads;
  const int64_t qp = a.q_stride, kp = a.kv_stride;
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    AttnItem w;
    int split = 0, k_beg = 0;
    if (KSPLIT) {
      const int64_t t = id / heads;
      split = (int)(t % ks.k_splits);
      attn_item((t / ks.k_splits) * heads + id % heads, nblk, heads, a.cu_q, a.cu_k, w);
    } else {
      attn_item(id, nblk, heads, a.cu_q, a.cu_k, w);
    }
    if (w.b0 >= w.len_q) continue;
    int k_end = w.len_k;
    if (KSPLIT) attn_key_share(w.len_k, ks.k_splits, split, k_beg, k_end);
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D;
    frag qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = load8<T>(q, qp, w.b0 + r, w.len_q, 16 * s + 8 * h);
    a_f32x16 acc[NMB];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mb][i] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int k0 = k_beg; k0 < k_end; k0 += kAttnBlock) {
      a_f32x16 st;
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) st = AFrag<T>::mfma(load8<T>(k, kp, k0 + r, w.len_k, 16 * s + 8 * h), qf[s], st);
      __syncthreads();  // the previous tile's reads of vt are done
      stage_transposed<T, D>(vt, v, kp, k0, w.len_k);
      float x[16];
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        x[i] = k0 + acc_row(i, h) < w.len_k ? st[i] * c2 : -INFINITY;
        mx = fmaxf(mx, x[i]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mn = fmaxf(m, mx);  // finite: key k0 is inside the sequence's keys
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
    if (KSPLIT) {
      // the share's state as it stands: an empty share leaves m = -inf, l = 0 and a zero accumulator
      if (row < w.len_q) {
        const int64_t idx = ((int64_t)split * ks.total_q + w.beg_q + row) * heads + w.hd;
        store_dcol_f32<D>(ks.o + idx * D, acc, h);
        if (h == 0) *reinterpret_cast<float2*>(ks.ml + 2 * idx) = make_float2(m, l);
      }
    } else if (row < w.len_q) {
      // l > 0 whenever the sequence has a key (the row maximum contributes exp2(0) = 1).  No key: the accumulator is
      // still zero and is stored as exact zeros, lse = -inf.
      const bool any = w.len_k > 0;
      const int64_t t = w.beg_q + row;
      store_dcol<T, D>(out + (t * heads + w.hd) * D, acc, any ? 1.f / l : 0.f, h);
      if (h == 0) lse[t * heads + w.hd] = any ? (m + __log2f(l)) * kLn2 : -INFINITY;
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

// dK, dV of one (sequence, 32-key block, head) - or, with SPLIT, of one share of that item's query blocks: item ids then
// are (sequence, key block, split, head) and the unscaled sums go to part [q_splits, total_k, 2, H, D] in fp32.
template <typename T, int D, bool SPLIT>
__global__ __launch_bounds__(64) void attn_bwd_dkdv_kernel(const AttnOperands<T> a, const T* __restrict__ dout,
                                                           const float* __restrict__ lse, const float* __restrict__ delta,
                                                           int64_t items, int nblk, float c2, float scale,
                                                           T* __restrict__ dk_out, T* __restrict__ dv_out, int64_t dkv_stride,
                                                           int q_splits, int64_t total_k, float* __restrict__ part) {
  typedef typename AFrag<T>::type frag;
  constexpr int NS = D / 16, NMB = (D + 31) / 32;
  __shared__ __attribute__((aligned(16))) T qt[NMB * 32 * kAttnPitch];
  __shared__ __attribute__((aligned(16))) T dot[NMB * 32 * kAttnPitch];
  __shared__ __attribute__((aligned(16))) float s_lse[kAttnBlock];
  __shared__ __attribute__((aligned(16))) float s_del[kAttnBlock];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int heads = a.heads;
  const int64_t qp = a.q_stride, kp = a.kv_stride, opitch = (int64_t)heads * D;
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    AttnItem w;
    int split = 0;
    if (SPLIT) {
      const int64_t t = id / heads;
      split = (int)(t % q_splits);
      attn_item((t / q_splits) * heads + id % heads, nblk, heads, a.cu_q, a.cu_k, w);
    } else {
      attn_item(id, nblk, heads, a.cu_q, a.cu_k, w);
    }
    if (w.b0 >= w.len_k) continue;
    // the query rows this wave sweeps: all of them, or split's share of the 32-row blocks (an empty share stores zeros)
    int q_beg = 0, q_end = w.len_q;
    if (SPLIT) {
      const int64_t nq = (w.len_q + kAttnBlock - 1) / kAttnBlock, per = (nq + q_splits - 1) / q_splits;
      const int64_t lo = split * per * kAttnBlock, hi = (split + 1) * per * kAttnBlock;
      q_beg = (int)(lo < w.len_q ? lo : w.len_q);
      q_end = (int)(hi < w.len_q ? hi : w.len_q);
    }
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D;
    const T* dO = dout + w.beg_q * opitch + (int64_t)w.hd * D;
    const int key = w.b0 + r;
    frag kf[NS], vf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      kf[s] = load8<T>(k, kp, key, w.len_k, 16 * s + 8 * h);
      vf[s] = load8<T>(v, kp, key, w.len_k, 16 * s + 8 * h);
    }
    a_f32x16 dk[NMB], dv[NMB];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) dk[mb][i] = dv[mb][i] = 0.f;
    for (int q0 = q_beg; q0 < q_end; q0 += kAttnBlock) {
      a_f32x16 sc, dp;
      frag qf[NS], df[NS];
#pragma unroll
      for (int i = 0; i < 16; ++i) sc[i] = dp[i] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        qf[s] = load8<T>(q, qp, q0 + r, w.len_q, 16 * s + 8 * h);
        df[s] = load8<T>(dO, opitch, q0 + r, w.len_q, 16 * s + 8 * h);
        sc = AFrag<T>::mfma(qf[s], kf[s], sc);
        dp = AFrag<T>::mfma(df[s], vf[s], dp);
      }
      __syncthreads();  // the previous block's reads of the images are done
      stage_frags<T, D>(qt, qf, r, h);
      stage_frags<T, D>(dot, df, r, h);
      {
        // this sequence has a key (b0 < len_k), so the forward's lse of its queries is finite; the test keeps an lse of
        // -inf (a caller's own buffer) out of the subtraction below all the same
        const int qr = q0 + r;
        const bool ok = qr < w.len_q;
        const int64_t t = w.beg_q + qr;
        if (h == 0) {
          const float L = ok ? lse[t * heads + w.hd] : 0.f;
          s_lse[r] = L > -INFINITY ? L * kLog2e : INFINITY;  // +inf: p = exp2(-inf) = 0
        } else {
          s_del[r] = ok ? delta[t * heads + w.hd] : 0.f;
        }
      }
      __syncthreads();
      // Rows of sc / dp are queries, the lane's column is its key.  Query rows past len_q carry Q = dO = 0, lse =
      // delta = 0: p = 1, dS = 0, and their dO^T / Q^T columns are zero, so they add nothing.  Keys past len_k: p = 0.
      float p[16], ds[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 L = *reinterpret_cast<const float4*>(s_lse + 8 * g + 4 * h);
        const float4 E = *reinterpret_cast<const float4*>(s_del + 8 * g + 4 * h);
        const float Lv[4] = {L.x, L.y, L.z, L.w}, Ev[4] = {E.x, E.y, E.z, E.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g + e;
          p[i] = key < w.len_k ? __builtin_amdgcn_exp2f(sc[i] * c2 - Lv[e]) : 0.f;
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
    if (key < w.len_k) {
      if (SPLIT) {
        float* dst = part + (((int64_t)split * total_k + w.beg_k + key) * 2 * heads + w.hd) * D;
        store_dcol_f32<D>(dst, dk, h);
        store_dcol_f32<D>(dst + (int64_t)heads * D, dv, h);
      } else {
        const int64_t off = (w.beg_k + key) * dkv_stride + (int64_t)w.hd * D;
        store_dcol<T, D>(dk_out + off, dk, scale, h);
        store_dcol<T, D>(dv_out + off, dv, 1.f, h);
      }
    }
  }
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

// dQ of one (sequence, 32-query block, head) - or, with KSPLIT, of one share of that item's keys (the forward's shares):
// P is recomputed from the final LSE, so the unscaled fp32 partials in ks.o only need adding (attn_dq_reduce_kernel).
template <typename T, int D, bool KSPLIT>
__global__ __launch_bounds__(64) void attn_bwd_dq_kernel(const AttnOperands<T> a, const T* __restrict__ dout,
                                                         const float* __restrict__ lse, const float* __restrict__ delta,
                                                         int64_t items, int nblk, float c2, float scale, T* __restrict__ dq_out,
                                                         int64_t dq_stride, const AttnKSplit ks) {
  typedef typename AFrag<T>::type frag;
  constexpr int NS = D / 16, NMB = (D + 31) / 32;
  __shared__ __attribute__((aligned(16))) T kt[NMB * 32 * kAttnPitch];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int heads = a.heads;
  const int64_t qp = a.q_stride, kp = a.kv_stride, opitch = (int64_t)heads * D;
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    AttnItem w;
    int split = 0, k_beg = 0;
    if (KSPLIT) {
      const int64_t t = id / heads;
      split = (int)(t % ks.k_splits);
      attn_item((t / ks.k_splits) * heads + id % heads, nblk, heads, a.cu_q, a.cu_k, w);
    } else {
      attn_item(id, nblk, heads, a.cu_q, a.cu_k, w);
    }
    if (w.b0 >= w.len_q) continue;
    int k_end = w.len_k;
    if (KSPLIT) attn_key_share(w.len_k, ks.k_splits, split, k_beg, k_end);
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D;
    const T* dO = dout + w.beg_q * opitch + (int64_t)w.hd * D;
    const int row = w.b0 + r;
    const bool ok = row < w.len_q;
    frag qf[NS], df[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      qf[s] = load8<T>(q, qp, row, w.len_q, 16 * s + 8 * h);
      df[s] = load8<T>(dO, opitch, row, w.len_q, 16 * s + 8 * h);
    }
    // lse = -inf marks a query with no key: its sweep below is empty and dq stays zero; +inf here (p = exp2(-inf) = 0)
    // keeps such a value out of the subtraction whatever the caller's buffer holds
    float L = ok ? lse[(w.beg_q + row) * heads + w.hd] : 0.f;
    L = L > -INFINITY ? L * kLog2e : INFINITY;
    const float E = ok ? delta[(w.beg_q + row) * heads + w.hd] : 0.f;
    a_f32x16 dq[NMB];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) dq[mb][i] = 0.f;
    for (int k0 = k_beg; k0 < k_end; k0 += kAttnBlock) {
      a_f32x16 st, dpt;
      frag kf[NS];
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = dpt[i] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        kf[s] = load8<T>(k, kp, k0 + r, w.len_k, 16 * s + 8 * h);
        st = AFrag<T>::mfma(kf[s], qf[s], st);
        dpt = AFrag<T>::mfma(load8<T>(v, kp, k0 + r, w.len_k, 16 * s + 8 * h), df[s], dpt);
      }
      __syncthreads();
      stage_frags<T, D>(kt, kf, r, h);
      // rows are keys, the lane's column its query; keys past len_k get p = 0 (their K, V rows were read as zeros)
      float ds[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = k0 + acc_row(i, h) < w.len_k ? __builtin_amdgcn_exp2f(st[i] * c2 - L) : 0.f;
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
    if (KSPLIT) {
      if (ok) store_dcol_f32<D>(ks.o + (((int64_t)split * ks.total_q + w.beg_q + row) * heads + w.hd) * D, dq, h);
    } else if (ok) {
      store_dcol<T, D>(dq_out + (w.beg_q + row) * dq_stride + (int64_t)w.hd * D, dq, scale, h);
    }
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

// ---- shared-tile variants: four waves per workgroup, every tile of the swept side staged once in LDS ------------------
// One tile is 32 rows x D elements = 4 D pieces of 16 bytes: thread c < 4 D of the workgroup owns piece (row c & 31,
// d-chunk c >> 5) - the walk of stage_transposed - loads it into a register while the previous tile is multiplied, and
// writes it to the other buffer afterwards (one barrier per tile).
constexpr int kAttnWaves = 4;
constexpr int kAttnWgRows = kAttnWaves * kAttnBlock;  // rows of a shared-tile work item
template <int D>
struct SharedTile {
  static constexpr int kRowPitch = D + 8;                       // row-major image: 16-B aligned rows, elements
  static constexpr int kRows = kAttnBlock * kRowPitch;          // elements of a row-major image
  static constexpr int kTr = ((D + 31) / 32) * 32 * kAttnPitch; // elements of a transposed image
};

template <typename T, int D>
__device__ __forceinline__ void put_rows(T* __restrict__ rows, const typename AFrag<T>::type& v, int row, int dch) {
  *reinterpret_cast<typename AFrag<T>::type*>(rows + row * SharedTile<D>::kRowPitch + 8 * dch) = v;
}
template <typename T>
__device__ __forceinline__ void put_tr(T* __restrict__ img, const typename AFrag<T>::type& v, int row, int dch) {
#pragma unroll
  for (int e = 0; e < 8; ++e) img[(8 * dch + e) * kAttnPitch + row] = v[e];
}
// The fragment load8 returns for (row r, d 16 s + 8 h .. + 7), from a row-major image.
template <typename T, int D>
__device__ __forceinline__ typename AFrag<T>::type get_row(const T* __restrict__ rows, int r, int s, int h) {
  return *reinterpret_cast<const typename AFrag<T>::type*>(rows + r * SharedTile<D>::kRowPitch + 16 * s + 8 * h);
}

template <typename T, int D, bool KSPLIT>
__global__ __launch_bounds__(256) void attn_fwd_shared_kernel(const AttnOperands<T> a, int64_t items, int nblk, float c2,
                                                              T* __restrict__ out, float* __restrict__ lse,
                                                              const AttnKSplit ks) {
  typedef typename AFrag<T>::type frag;
  typedef SharedTile<D> Tile;
  constexpr int NS = D / 16, NMB = (D + 31) / 32;
  __shared__ __attribute__((aligned(16))) T kr[2][Tile::kRows];
  __shared__ __attribute__((aligned(16))) T vt[2][Tile::kTr];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int srow = tid & 31, sdch = tid >> 5;
  const bool stager = tid < 4 * D;
  const int heads = a.heads;
  const int64_t qp = a.q_stride, kp = a.kv_stride;
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    AttnItem w;
    int split = 0, k_beg = 0;
    if (KSPLIT) {
      const int64_t t = id / heads;
      split = (int)(t % ks.k_splits);
      attn_item((t / ks.k_splits) * heads + id % heads, nblk, heads, a.cu_q, a.cu_k, w, kAttnWgRows);
    } else {
      attn_item(id, nblk, heads, a.cu_q, a.cu_k, w, kAttnWgRows);
    }
    if (w.b0 >= w.len_q) continue;  // (the same for every wave of the workgroup)
    int k_end = w.len_k;
    if (KSPLIT) attn_key_share(w.len_k, ks.k_splits, split, k_beg, k_end);
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D;
    const int rb = w.b0 + kAttnBlock * wave;  // this wave's rows; past the end they are zeros and nothing is stored
    frag qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = load8<T>(q, qp, rb + r, w.len_q, 16 * s + 8 * h);
    a_f32x16 acc[NMB];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mb][i] = 0.f;
    float m = -INFINITY, l = 0.f;
    frag kreg, vreg;
    if (stager && k_beg < k_end) {
      put_rows<T, D>(kr[0], load8<T>(k, kp, k_beg + srow, w.len_k, 8 * sdch), srow, sdch);
      put_tr<T>(vt[0], load8<T>(v, kp, k_beg + srow, w.len_k, 8 * sdch), srow, sdch);
    }
    __syncthreads();
    for (int k0 = k_beg, cur = 0; k0 < k_end; k0 += kAttnBlock, cur ^= 1) {
      const bool more = stager && k0 + kAttnBlock < k_end;
      if (more) {  // the next tile's loads are in flight during this tile's MFMAs
        kreg = load8<T>(k, kp, k0 + kAttnBlock + srow, w.len_k, 8 * sdch);
        vreg = load8<T>(v, kp, k0 + kAttnBlock + srow, w.len_k, 8 * sdch);
      }
      a_f32x16 st;
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) st = AFrag<T>::mfma(get_row<T, D>(kr[cur], r, s, h), qf[s], st);
      float x[16];
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        x[i] = k0 + acc_row(i, h) < w.len_k ? st[i] * c2 : -INFINITY;
        mx = fmaxf(mx, x[i]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mn = fmaxf(m, mx);
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
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const frag pf = acc_frag<T>(x, s);
#pragma unroll
        for (int mb = 0; mb < NMB; ++mb) acc[mb] = AFrag<T>::mfma(read_tr<T>(vt[cur], mb, s, r, h), pf, acc[mb]);
      }
      if (more) {
        put_rows<T, D>(kr[cur ^ 1], kreg, srow, sdch);
        put_tr<T>(vt[cur ^ 1], vreg, srow, sdch);
      }
      __syncthreads();  // the next tile is staged, and this tile's reads are done before its buffer is written again
    }
    const int row = rb + r;
    if (KSPLIT) {
      if (row < w.len_q) {
        const int64_t idx = ((int64_t)split * ks.total_q + w.beg_q + row) * heads + w.hd;
        store_dcol_f32<D>(ks.o + idx * D, acc, h);
        if (h == 0) *reinterpret_cast<float2*>(ks.ml + 2 * idx) = make_float2(m, l);
      }
    } else if (row < w.len_q) {
      const bool any = w.len_k > 0;
      const int64_t t = w.beg_q + row;
      store_dcol<T, D>(out + (t * heads + w.hd) * D, acc, any ? 1.f / l : 0.f, h);
      if (h == 0) lse[t * heads + w.hd] = any ? (m + __log2f(l)) * kLn2 : -INFINITY;
    }
  }
}

// dQ of one (sequence, 128-query block, [split,] head): K and V rows and the K^T image staged once per key tile.  KSPLIT as
// in attn_bwd_dq_kernel (same shares, same partial layout).
template <typename T, int D, bool KSPLIT>
__global__ __launch_bounds__(256) void attn_bwd_dq_shared_kernel(const AttnOperands<T> a, const T* __restrict__ dout,
                                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 int64_t items, int nblk, float c2, float scale,
                                                                 T* __restrict__ dq_out, int64_t dq_stride,
                                                                 const AttnKSplit ks) {
  typedef typename AFrag<T>::type frag;
  typedef SharedTile<D> Tile;
  constexpr int NS = D / 16, NMB = (D + 31) / 32;
  __shared__ __attribute__((aligned(16))) T kr[2][Tile::kRows];
  __shared__ __attribute__((aligned(16))) T vr[2][Tile::kRows];
  __shared__ __attribute__((aligned(16))) T kt[2][Tile::kTr];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int srow = tid & 31, sdch = tid >> 5;
  const bool stager = tid < 4 * D;
  const int heads = a.heads;
  const int64_t qp = a.q_stride, kp = a.kv_stride, opitch = (int64_t)heads * D;
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    AttnItem w;
    int split = 0, k_beg = 0;
    if (KSPLIT) {
      const int64_t t = id / heads;
      split = (int)(t % ks.k_splits);
      attn_item((t / ks.k_splits) * heads + id % heads, nblk, heads, a.cu_q, a.cu_k, w, kAttnWgRows);
    } else {
      attn_item(id, nblk, heads, a.cu_q, a.cu_k, w, kAttnWgRows);
    }
    if (w.b0 >= w.len_q) continue;
    int k_end = w.len_k;
    if (KSPLIT) attn_key_share(w.len_k, ks.k_splits, split, k_beg, k_end);
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D;
    const T* dO = dout + w.beg_q * opitch + (int64_t)w.hd * D;
    const int row = w.b0 + kAttnBlock * wave + r;
    const bool ok = row < w.len_q;
    frag qf[NS], df[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      qf[s] = load8<T>(q, qp, row, w.len_q, 16 * s + 8 * h);
      df[s] = load8<T>(dO, opitch, row, w.len_q, 16 * s + 8 * h);
    }
    float L = ok ? lse[(w.beg_q + row) * heads + w.hd] : 0.f;
    L = L > -INFINITY ? L * kLog2e : INFINITY;
    const float E = ok ? delta[(w.beg_q + row) * heads + w.hd] : 0.f;
    a_f32x16 dq[NMB];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) dq[mb][i] = 0.f;
    frag kreg, vreg;
    if (stager && k_beg < k_end) {
      kreg = load8<T>(k, kp, k_beg + srow, w.len_k, 8 * sdch);
      put_rows<T, D>(kr[0], kreg, srow, sdch);
      put_tr<T>(kt[0], kreg, srow, sdch);
      put_rows<T, D>(vr[0], load8<T>(v, kp, k_beg + srow, w.len_k, 8 * sdch), srow, sdch);
    }
    __syncthreads();
    for (int k0 = k_beg, cur = 0; k0 < k_end; k0 += kAttnBlock, cur ^= 1) {
      const bool more = stager && k0 + kAttnBlock < k_end;
      if (more) {
        kreg = load8<T>(k, kp, k0 + kAttnBlock + srow, w.len_k, 8 * sdch);
        vreg = load8<T>(v, kp, k0 + kAttnBlock + srow, w.len_k, 8 * sdch);
      }
      a_f32x16 st, dpt;
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = dpt[i] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        st = AFrag<T>::mfma(get_row<T, D>(kr[cur], r, s, h), qf[s], st);
        dpt = AFrag<T>::mfma(get_row<T, D>(vr[cur], r, s, h), df[s], dpt);
      }
      float ds[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = k0 + acc_row(i, h) < w.len_k ? __builtin_amdgcn_exp2f(st[i] * c2 - L) : 0.f;
        ds[i] = p * (dpt[i] - E);
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const frag dsf = acc_frag<T>(ds, s);
#pragma unroll
        for (int mb = 0; mb < NMB; ++mb) dq[mb] = AFrag<T>::mfma(read_tr<T>(kt[cur], mb, s, r, h), dsf, dq[mb]);
      }
      if (more) {
        put_rows<T, D>(kr[cur ^ 1], kreg, srow, sdch);
        put_tr<T>(kt[cur ^ 1], kreg, srow, sdch);
        put_rows<T, D>(vr[cur ^ 1], vreg, srow, sdch);
      }
      __syncthreads();
    }
    if (KSPLIT) {
      if (ok) store_dcol_f32<D>(ks.o + (((int64_t)split * ks.total_q + w.beg_q + row) * heads + w.hd) * D, dq, h);
    } else if (ok) {
      store_dcol<T, D>(dq_out + (w.beg_q + row) * dq_stride + (int64_t)w.hd * D, dq, scale, h);
    }
  }
}

// dK, dV of one (sequence, 128-key block, [split,] head): Q and dO rows, their transposed images, lse and delta staged
// once per query tile.  SPLIT as in attn_bwd_dkdv_kernel (same shares, same partial layout).
template <typename T, int D, bool SPLIT>
__global__ __launch_bounds__(256) void attn_bwd_dkdv_shared_kernel(const AttnOperands<T> a, const T* __restrict__ dout,
                                                                   const float* __restrict__ lse, const float* __restrict__ delta,
                                                                   int64_t items, int nblk, float c2, float scale,
                                                                   T* __restrict__ dk_out, T* __restrict__ dv_out,
                                                                   int64_t dkv_stride, int q_splits, int64_t total_k,
                                                                   float* __restrict__ part) {
  typedef typename AFrag<T>::type frag;
  typedef SharedTile<D> Tile;
  constexpr int NS = D / 16, NMB = (D + 31) / 32;
  __shared__ __attribute__((aligned(16))) T qr[2][Tile::kRows];
  __shared__ __attribute__((aligned(16))) T dr[2][Tile::kRows];
  __shared__ __attribute__((aligned(16))) T qt[2][Tile::kTr];
  __shared__ __attribute__((aligned(16))) T dot[2][Tile::kTr];
  __shared__ __attribute__((aligned(16))) float s_lse[2][kAttnBlock];
  __shared__ __attribute__((aligned(16))) float s_del[2][kAttnBlock];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int srow = tid & 31, sdch = tid >> 5;
  const bool stager = tid < 4 * D;
  const int heads = a.heads;
  const int64_t qp = a.q_stride, kp = a.kv_stride, opitch = (int64_t)heads * D;
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    AttnItem w;
    int split = 0;
    if (SPLIT) {
      const int64_t t = id / heads;
      split = (int)(t % q_splits);
      attn_item((t / q_splits) * heads + id % heads, nblk, heads, a.cu_q, a.cu_k, w, kAttnWgRows);
    } else {
      attn_item(id, nblk, heads, a.cu_q, a.cu_k, w, kAttnWgRows);
    }
    if (w.b0 >= w.len_k) continue;
    int q_beg = 0, q_end = w.len_q;
    if (SPLIT) {
      const int64_t nq = (w.len_q + kAttnBlock - 1) / kAttnBlock, per = (nq + q_splits - 1) / q_splits;
      const int64_t lo = split * per * kAttnBlock, hi = (split + 1) * per * kAttnBlock;
      q_beg = (int)(lo < w.len_q ? lo : w.len_q);
      q_end = (int)(hi < w.len_q ? hi : w.len_q);
    }
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D;
    const T* dO = dout + w.beg_q * opitch + (int64_t)w.hd * D;
    const int key = w.b0 + kAttnBlock * wave + r;
    frag kf[NS], vf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      kf[s] = load8<T>(k, kp, key, w.len_k, 16 * s + 8 * h);
      vf[s] = load8<T>(v, kp, key, w.len_k, 16 * s + 8 * h);
    }
    a_f32x16 dk[NMB], dv[NMB];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) dk[mb][i] = dv[mb][i] = 0.f;
    // the staged scalar of thread tid < 32: lse (exp2 domain, +inf for a query without a key) of query row q0 + tid; of
    // 32 <= tid < 64: delta of row q0 + tid - 32
    auto load_stat = [&](int q0) -> float {
      const int qrow = q0 + srow;
      const bool ok = qrow < w.len_q;
      const int64_t t = w.beg_q + qrow;
      if (tid < kAttnBlock) {
        const float L = ok ? lse[t * heads + w.hd] : 0.f;
        return L > -INFINITY ? L * kLog2e : INFINITY;
      }
      return ok ? delta[t * heads + w.hd] : 0.f;
    };
    auto put_stat = [&](int buf, float x) {
      if (tid < kAttnBlock) s_lse[buf][srow] = x;
      else s_del[buf][srow] = x;
    };
    frag qreg, dreg;
    float stat = 0.f;
    if (q_beg < q_end) {
      if (stager) {
        qreg = load8<T>(q, qp, q_beg + srow, w.len_q, 8 * sdch);
        dreg = load8<T>(dO, opitch, q_beg + srow, w.len_q, 8 * sdch);
        put_rows<T, D>(qr[0], qreg, srow, sdch);
        put_tr<T>(qt[0], qreg, srow, sdch);
        put_rows<T, D>(dr[0], dreg, srow, sdch);
        put_tr<T>(dot[0], dreg, srow, sdch);
      }
      if (tid < 2 * kAttnBlock) put_stat(0, load_stat(q_beg));
    }
    __syncthreads();
    for (int q0 = q_beg, cur = 0; q0 < q_end; q0 += kAttnBlock, cur ^= 1) {
      const bool more = q0 + kAttnBlock < q_end;
      if (more) {
        if (stager) {
          qreg = load8<T>(q, qp, q0 + kAttnBlock + srow, w.len_q, 8 * sdch);
          dreg = load8<T>(dO, opitch, q0 + kAttnBlock + srow, w.len_q, 8 * sdch);
        }
        if (tid < 2 * kAttnBlock) stat = load_stat(q0 + kAttnBlock);
      }
      a_f32x16 sc, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) sc[i] = dp[i] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        sc = AFrag<T>::mfma(get_row<T, D>(qr[cur], r, s, h), kf[s], sc);
        dp = AFrag<T>::mfma(get_row<T, D>(dr[cur], r, s, h), vf[s], dp);
      }
      float p[16], ds[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 L = *reinterpret_cast<const float4*>(s_lse[cur] + 8 * g + 4 * h);
        const float4 E = *reinterpret_cast<const float4*>(s_del[cur] + 8 * g + 4 * h);
        const float Lv[4] = {L.x, L.y, L.z, L.w}, Ev[4] = {E.x, E.y, E.z, E.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g + e;
          p[i] = key < w.len_k ? __builtin_amdgcn_exp2f(sc[i] * c2 - Lv[e]) : 0.f;
          ds[i] = p[i] * (dp[i] - Ev[e]);
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const frag pf = acc_frag<T>(p, s), dsf = acc_frag<T>(ds, s);
#pragma unroll
        for (int mb = 0; mb < NMB; ++mb) {
          dv[mb] = AFrag<T>::mfma(read_tr<T>(dot[cur], mb, s, r, h), pf, dv[mb]);
          dk[mb] = AFrag<T>::mfma(read_tr<T>(qt[cur], mb, s, r, h), dsf, dk[mb]);
        }
      }
      if (more) {
        if (stager) {
          put_rows<T, D>(qr[cur ^ 1], qreg, srow, sdch);
          put_tr<T>(qt[cur ^ 1], qreg, srow, sdch);
          put_rows<T, D>(dr[cur ^ 1], dreg, srow, sdch);
          put_tr<T>(dot[cur ^ 1], dreg, srow, sdch);
        }
        if (tid < 2 * kAttnBlock) put_stat(cur ^ 1, stat);
      }
      __syncthreads();
    }
    if (key < w.len_k) {
      if (SPLIT) {
        float* dst = part + (((int64_t)split * total_k + w.beg_k + key) * 2 * heads + w.hd) * D;
        store_dcol_f32<D>(dst, dk, h);
        store_dcol_f32<D>(dst + (int64_t)heads * D, dv, h);
      } else {
        const int64_t off = (w.beg_k + key) * dkv_stride + (int64_t)w.hd * D;
        store_dcol<T, D>(dk_out + off, dk, scale, h);
        store_dcol<T, D>(dv_out + off, dv, 1.f, h);
      }
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
// One call's operands and sizes, already checked.
struct AttnCall {
  const void *q, *k, *v;
  int64_t q_stride, kv_stride;
  const int32_t *cu_q, *cu_k;
  int64_t num_seqs, total_q, total_k;
  int heads, max_q, max_k;
  float scale;
};

static inline int attn_blocks(int max_seqlen) { return (max_seqlen + kAttnBlock - 1) / kAttnBlock; }
static inline unsigned attn_grid(int64_t items) { return (unsigned)(items < kAttnMaxGrid ? items : kAttnMaxGrid); }

template <typename T>
static AttnOperands<T> attn_operands(const AttnCall& c) {
  return AttnOperands<T>{(const T*)c.q, (const T*)c.k, (const T*)c.v, c.q_stride, c.kv_stride, c.cu_q, c.cu_k, c.heads};
}

static inline int attn_wg_blocks(int max_seqlen) { return (max_seqlen + kAttnWgRows - 1) / kAttnWgRows; }

// The AUTO rule (see wcn.h; the measurements behind it: docs/OPTIMISATION_LOG.md).
constexpr int kAttnSharedMinSweep = 512;  // rows of the swept side from which the shared kernels were measured ahead
static int attn_variant(const AttnCall& c, int variant, int direction) {
  if (variant != WCN_ATTN_AUTO) return variant;
  return wcn_attn_varlen_variant(c.num_seqs, c.max_q, c.max_k, c.heads, direction);
}

// k_splits > 1: the split-key kernels into the partials `ks`, then the combine; 1: the unsplit kernels, as ever.
template <typename T, int D>
static int attn_fwd_t(const AttnCall& c, void* out, float* lse, int variant, const AttnKSplit& ks, hipStream_t s) {
  const bool shared = attn_variant(c, variant, 0) == WCN_ATTN_SHARED;
  const int nblk = shared ? attn_wg_blocks(c.max_q) : attn_blocks(c.max_q);
  const dim3 wg(shared ? 64 * kAttnWaves : 64);
  const int64_t items = c.num_seqs * nblk * c.heads * ks.k_splits;
  const AttnOperands<T> a = attn_operands<T>(c);
  const float c2 = c.scale * kLog2e;
  if (items > 0) {
    if (ks.k_splits > 1) {
      if (shared)
        hipLaunchKernelGGL((attn_fwd_shared_kernel<T, D, true>), dim3(attn_grid(items)), wg, 0, s, a, items, nblk, c2, (T*)out,
                           lse, ks);
      else
        hipLaunchKernelGGL((attn_fwd_kernel<T, D, true>), dim3(attn_grid(items)), wg, 0, s, a, items, nblk, c2, (T*)out, lse, ks);
      const int64_t n = c.total_q * c.heads * (D / 4);
      hipLaunchKernelGGL((attn_fwd_combine_kernel<T, D>), dim3(attn_grid((n + 255) / 256)), dim3(256), 0, s, ks, c.cu_q,
                         c.num_seqs, c.heads, (T*)out, lse);
    } else if (shared) {
      hipLaunchKernelGGL((attn_fwd_shared_kernel<T, D, false>), dim3(attn_grid(items)), wg, 0, s, a, items, nblk, c2, (T*)out,
                         lse, ks);
    } else {
      hipLaunchKernelGGL((attn_fwd_kernel<T, D, false>), dim3(attn_grid(items)), wg, 0, s, a, items, nblk, c2, (T*)out, lse, ks);
    }
  }
  return hipGetLastError() == hipSuccess ? WCN_SUCCESS : WCN_ERROR_KERNEL_EXECUTION;
}

template <typename T, int D>
static int attn_bwd_t(const AttnCall& c, const void* dout, const void* out, const float* lse, void* dq, int64_t dq_stride,
                      void* dk, void* dv, int64_t dkv_stride, int q_splits, float* part, float* delta, int variant,
                      const AttnKSplit& ks, hipStream_t s) {
  const AttnOperands<T> a = attn_operands<T>(c);
  const float c2 = c.scale * kLog2e;
  const int64_t rows = c.total_q * c.heads;
  const bool shared = attn_variant(c, variant, 1) == WCN_ATTN_SHARED;
  const int nblk_q = shared ? attn_wg_blocks(c.max_q) : attn_blocks(c.max_q);
  const int nblk_k = shared ? attn_wg_blocks(c.max_k) : attn_blocks(c.max_k);
  const dim3 wg(shared ? 64 * kAttnWaves : 64);
  const int64_t items_q = c.num_seqs * nblk_q * c.heads, items_k = c.num_seqs * nblk_k * c.heads;
  if (rows > 0)
    hipLaunchKernelGGL((attn_delta_kernel<T, D>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, (const T*)dout,
                       (const T*)out, rows, delta);
  if (items_k > 0 && c.total_k > 0) {
    if (q_splits > 1) {
      if (shared)
        hipLaunchKernelGGL((attn_bwd_dkdv_shared_kernel<T, D, true>), dim3(attn_grid(items_k * q_splits)), wg, 0, s, a,
                           (const T*)dout, lse, (const float*)delta, items_k * q_splits, nblk_k, c2, c.scale, (T*)dk, (T*)dv,
                           dkv_stride, q_splits, c.total_k, part);
      else
        hipLaunchKernelGGL((attn_bwd_dkdv_kernel<T, D, true>), dim3(attn_grid(items_k * q_splits)), wg, 0, s, a,
                           (const T*)dout, lse, (const float*)delta, items_k * q_splits, nblk_k, c2, c.scale, (T*)dk, (T*)dv,
                           dkv_stride, q_splits, c.total_k, part);
      const int64_t n = c.total_k * 2 * c.heads * (D / 4);
      hipLaunchKernelGGL((attn_dkdv_reduce_kernel<T, D>), dim3(attn_grid((n + 255) / 256)), dim3(256), 0, s,
                         (const float*)part, c.cu_k, c.num_seqs, c.total_k, c.heads, q_splits, c.scale, (T*)dk, (T*)dv,
                         dkv_stride);
    } else if (shared) {
      hipLaunchKernelGGL((attn_bwd_dkdv_shared_kernel<T, D, false>), dim3(attn_grid(items_k)), wg, 0, s, a, (const T*)dout, lse,
                         (const float*)delta, items_k, nblk_k, c2, c.scale, (T*)dk, (T*)dv, dkv_stride, 1, c.total_k,
                         (float*)nullptr);
    } else {
      hipLaunchKernelGGL((attn_bwd_dkdv_kernel<T, D, false>), dim3(attn_grid(items_k)), wg, 0, s, a, (const T*)dout, lse,
                         (const float*)delta, items_k, nblk_k, c2, c.scale, (T*)dk, (T*)dv, dkv_stride, 1, c.total_k,
                         (float*)nullptr);
    }
  }
  if (items_q > 0 && c.total_q > 0) {
    if (ks.k_splits > 1) {
      const int64_t items = items_q * ks.k_splits;
      if (shared)
        hipLaunchKernelGGL((attn_bwd_dq_shared_kernel<T, D, true>), dim3(attn_grid(items)), wg, 0, s, a, (const T*)dout, lse,
                           (const float*)delta, items, nblk_q, c2, c.scale, (T*)dq, dq_stride, ks);
      else
        hipLaunchKernelGGL((attn_bwd_dq_kernel<T, D, true>), dim3(attn_grid(items)), wg, 0, s, a, (const T*)dout, lse,
                           (const float*)delta, items, nblk_q, c2, c.scale, (T*)dq, dq_stride, ks);
      const int64_t n = c.total_q * c.heads * (D / 4);
      hipLaunchKernelGGL((attn_dq_reduce_kernel<T, D>), dim3(attn_grid((n + 255) / 256)), dim3(256), 0, s, ks, c.cu_q,
                         c.num_seqs, c.heads, c.scale, (T*)dq, dq_stride);
    } else if (shared) {
      hipLaunchKernelGGL((attn_bwd_dq_shared_kernel<T, D, false>), dim3(attn_grid(items_q)), wg, 0, s, a, (const T*)dout, lse,
                         (const float*)delta, items_q, nblk_q, c2, c.scale, (T*)dq, dq_stride, ks);
    } else {
      hipLaunchKernelGGL((attn_bwd_dq_kernel<T, D, false>), dim3(attn_grid(items_q)), wg, 0, s, a, (const T*)dout, lse,
                         (const float*)delta, items_q, nblk_q, c2, c.scale, (T*)dq, dq_stride, ks);
    }
  }
  return hipGetLastError() == hipSuccess ? WCN_SUCCESS : WCN_ERROR_KERNEL_EXECUTION;
}

static const AttnKSplit kAttnNoKSplit{1, 0, nullptr, nullptr};

static int attn_fwd_dispatch(const AttnCall& c, int head_dim, int dtype, void* out, float* lse, int variant, hipStream_t s,
                             const AttnKSplit& ks = kAttnNoKSplit) {
  return with_dtype16(dtype, [&](auto t) {
    using T = decltype(t);
    switch (head_dim) {
      case 16: return attn_fwd_t<T, 16>(c, out, lse, variant, ks, s);
      case 32: return attn_fwd_t<T, 32>(c, out, lse, variant, ks, s);
      default: return attn_fwd_t<T, 64>(c, out, lse, variant, ks, s);
    }
  });
}

static int attn_bwd_dispatch(const AttnCall& c, int head_dim, int dtype, const void* dout, const void* out, const float* lse,
                             void* dq, int64_t dq_stride, void* dk, void* dv, int64_t dkv_stride, int q_splits, float* part,
                             float* delta, int variant, hipStream_t s, const AttnKSplit& ks = kAttnNoKSplit) {
  return with_dtype16(dtype, [&](auto t) {
    using T = decltype(t);
    switch (head_dim) {
      case 16: return attn_bwd_t<T, 16>(c, dout, out, lse, dq, dq_stride, dk, dv, dkv_stride, q_splits, part, delta, variant, ks, s);
      case 32: return attn_bwd_t<T, 32>(c, dout, out, lse, dq, dq_stride, dk, dv, dkv_stride, q_splits, part, delta, variant, ks, s);
      default: return attn_bwd_t<T, 64>(c, dout, out, lse, dq, dq_stride, dk, dv, dkv_stride, q_splits, part, delta, variant, ks, s);
    }
  });
}

// Shared argument checks of both directions of the packed form.  Returns WCN_SUCCESS, an error, or 1 = valid but nothing
// to launch.
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

// The packed tensor as three operands: slots of one [T, 3, H, D], one boundary array for both sides.
static AttnCall attn_packed_call(const void* qkv, const int32_t* cu, int64_t num_seqs, int64_t total, int32_t heads,
                                 int32_t head_dim, int32_t max_seqlen, float scale, int32_t esize) {
  const int64_t hd = (int64_t)heads * head_dim;
  const char* base = (const char*)qkv;
  return AttnCall{base, base + hd * esize, base + 2 * hd * esize, 3 * hd, 3 * hd, cu, cu, num_seqs, total, total, heads,
                  max_seqlen, max_seqlen, scale};
}


// Checks of the separate-operand form (both directions).  Same return convention as attn_check; "nothing to launch" is
// left to the caller, which knows what each direction writes.
static int attn_kv_check(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride, const int32_t* cu_q,
                         const int32_t* cu_k, int64_t num_seqs, int64_t total_q, int64_t total_k, int32_t heads,
                         int32_t head_dim, int32_t max_q, int32_t max_k, float scale, int32_t dtype) {
  if (num_seqs < 0 || total_q < 0 || total_k < 0 || heads < 1 || head_dim < 1 || max_q < 0 || max_k < 0 || !(scale == scale))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (num_seqs > 0 && (!cu_q || !cu_k)) return WCN_ERROR_INVALID_PARAMETERS;
  if ((total_q > 0 && !q) || (total_k > 0 && (!k || !v))) return WCN_ERROR_INVALID_PARAMETERS;
  if (total_q > INT32_MAX || total_k > INT32_MAX) return WCN_ERROR_INVALID_PARAMETERS;  // cu_* are int32
  if (!wcn_attn_varlen_supported(head_dim, dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  const int64_t hd = (int64_t)heads * head_dim;
  if (q_stride < hd || kv_stride < hd || (q_stride & 7) || (kv_stride & 7)) return WCN_ERROR_INVALID_PARAMETERS;
  if (!aligned_to(q, 16) || !aligned_to(k, 16) || !aligned_to(v, 16)) return WCN_ERROR_INVALID_PARAMETERS;
  return WCN_SUCCESS;
}

// The split rule of the dK/dV sweep (see wcn.h).  Measured on an MI355X: docs/OPTIMISATION_LOG.md.
constexpr int64_t kAttnSplitTargetWaves = 4096;          // (sequence, key block, split, head) waves worth launching
constexpr int kAttnSplitMinBlocks = 16;                  // query blocks a split sweeps at the least
constexpr int kAttnSplitMax = 16;
constexpr int64_t kAttnSplitPartCap = 256LL << 20;       // bytes of partials the rule may ask for (at head_dim 64)

// The split rule of the key sweep of the forward and of dQ (see wcn.h).  Measured on an MI355X: docs/OPTIMISATION_LOG.md.
constexpr int64_t kAttnKSplitTargetItems = 4096;         // (sequence, 128-query block, split, head) workgroups worth launching
// 32-key blocks a split sweeps at the least.  Set by a constraint, not by the table: 17 is the least value that leaves the
// 1 025-key shapes of the existing tests at one split (tests/test_attention_ksplit_api.py); the measured best at 2 000 keys
// is 4 - 8 splits, 8 - 16 blocks each.
constexpr int kAttnKSplitMinBlocks = 17;
constexpr int kAttnKSplitMax = 64;
constexpr int64_t kAttnKSplitPartCap = 256LL << 20;      // bytes of partials the rule may ask for (at head_dim 64)

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
  const AttnCall c = attn_packed_call(qkv, cu_seqlens, num_seqs, total, heads, head_dim, max_seqlen, softmax_scale, 2);
  return attn_fwd_dispatch(c, head_dim, dtype, out, lse, WCN_ATTN_AUTO, (hipStream_t)stream);
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
  const AttnCall c = attn_packed_call(qkv, cu_seqlens, num_seqs, total, heads, head_dim, max_seqlen, softmax_scale, 2);
  const int64_t hd = (int64_t)heads * head_dim;
  char* d = (char*)dqkv;
  return attn_bwd_dispatch(c, head_dim, dtype, dout, out, lse, d, 3 * hd, d + 2 * hd, d + 4 * hd, 3 * hd, 1, nullptr,
                           (float*)workspace, WCN_ATTN_AUTO, (hipStream_t)stream);
}

int32_t wcn_attn_varlen_kv_splits(int64_t num_seqs, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t heads) {
  if (num_seqs < 1 || max_seqlen_q < 1 || max_seqlen_k < 1 || heads < 1) return 1;
  const int64_t base = num_seqs * attn_blocks(max_seqlen_k) * heads;
  int64_t s = (kAttnSplitTargetWaves + base - 1) / base;
  const int64_t by_blocks = attn_blocks(max_seqlen_q) / kAttnSplitMinBlocks;
  const int64_t by_bytes = kAttnSplitPartCap / (num_seqs * max_seqlen_k * 2 * heads * 64 * (int64_t)sizeof(float));
  if (s > by_blocks) s = by_blocks;
  if (s > by_bytes) s = by_bytes;
  if (s > kAttnSplitMax) s = kAttnSplitMax;
  return s < 1 ? 1 : (int32_t)s;
}

size_t wcn_attn_varlen_kv_workspace_bytes(int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim, int32_t q_splits) {
  if (total_q < 0 || total_k < 0 || heads < 0 || head_dim < 0) return 0;
  size_t bytes = (size_t)total_q * (size_t)heads * sizeof(float);
  if (q_splits > 1) bytes += (size_t)q_splits * (size_t)total_k * 2 * (size_t)heads * (size_t)head_dim * sizeof(float);
  return bytes;
}

static bool attn_variant_ok(int32_t v) { return v == WCN_ATTN_AUTO || v == WCN_ATTN_ONE_WAVE || v == WCN_ATTN_SHARED; }

int32_t wcn_attn_varlen_variant(int64_t num_seqs, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t heads, int32_t direction) {
  if (num_seqs < 1 || max_seqlen_q < 1 || max_seqlen_k < 1 || heads < 1) return WCN_ATTN_ONE_WAVE;
  // the forward sweeps the keys of a query block; of the backward's two kernels dQ sweeps the keys, dK/dV the queries
  const int sweep = direction == 0 ? max_seqlen_k : (max_seqlen_q > max_seqlen_k ? max_seqlen_q : max_seqlen_k);
  return sweep >= kAttnSharedMinSweep ? WCN_ATTN_SHARED : WCN_ATTN_ONE_WAVE;
}

int wcn_attn_varlen_kv_fwd(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                           const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs, int64_t total_q, int64_t total_k,
                           int32_t heads, int32_t head_dim, int32_t max_seqlen_q, int32_t max_seqlen_k, float softmax_scale,
                           int32_t dtype, void* out, float* lse, wcn_stream_t stream) {
  return wcn_attn_varlen_kv_fwd_v(q, q_stride, k, v, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, head_dim,
                                  max_seqlen_q, max_seqlen_k, softmax_scale, dtype, out, lse, WCN_ATTN_AUTO, stream);
}

int wcn_attn_varlen_kv_fwd_v(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                             const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs, int64_t total_q, int64_t total_k,
                             int32_t heads, int32_t head_dim, int32_t max_seqlen_q, int32_t max_seqlen_k, float softmax_scale,
                             int32_t dtype, void* out, float* lse, int32_t variant, wcn_stream_t stream) {
  return wcn_attn_varlen_kv_fwd_s(q, q_stride, k, v, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, head_dim,
                                  max_seqlen_q, max_seqlen_k, softmax_scale, dtype, out, lse, variant, 1, nullptr, 0, stream);
}

int32_t wcn_attn_varlen_k_splits(int64_t num_seqs, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t heads,
                                 int32_t direction) {
  (void)direction;  // the forward and dQ sweep the same keys from the same work items: one rule for both
  if (num_seqs < 1 || max_seqlen_q < 1 || max_seqlen_k < 1 || heads < 1) return 1;
  // A sweep long enough to split (2 * kAttnKSplitMinBlocks blocks >= kAttnSharedMinSweep keys) runs the shared kernels
  // under WCN_ATTN_AUTO, so the unsplit launch is counted in their 128-query work items whatever variant is forced.
  const int64_t base = num_seqs * attn_wg_blocks(max_seqlen_q) * heads;
  int64_t s = (kAttnKSplitTargetItems + base - 1) / base;
  const int64_t by_blocks = attn_blocks(max_seqlen_k) / kAttnKSplitMinBlocks;
  const int64_t by_bytes = kAttnKSplitPartCap / (num_seqs * max_seqlen_q * heads * (64 + 2) * (int64_t)sizeof(float));
  if (s > by_blocks) s = by_blocks;
  if (s > by_bytes) s = by_bytes;
  if (s > kAttnKSplitMax) s = kAttnKSplitMax;
  return s < 1 ? 1 : (int32_t)s;
}

size_t wcn_attn_varlen_ksplit_workspace_bytes(int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim,
                                              int32_t q_splits, int32_t k_splits, int32_t direction) {
  if (total_q < 0 || total_k < 0 || heads < 0 || head_dim < 0) return 0;
  const size_t rows = (size_t)total_q * (size_t)heads;
  const size_t ks = k_splits > 1 ? (size_t)k_splits : 0;
  if (direction == 0) return ks * rows * ((size_t)head_dim + 2) * sizeof(float);
  return wcn_attn_varlen_kv_workspace_bytes(total_q, total_k, heads, head_dim, q_splits) +
         ks * rows * (size_t)head_dim * sizeof(float);
}

int wcn_attn_varlen_kv_fwd_s(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                             const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs, int64_t total_q, int64_t total_k,
                             int32_t heads, int32_t head_dim, int32_t max_seqlen_q, int32_t max_seqlen_k, float softmax_scale,
                             int32_t dtype, void* out, float* lse, int32_t variant, int32_t k_splits, void* workspace,
                             size_t workspace_bytes, wcn_stream_t stream) {
  if (!attn_variant_ok(variant) || k_splits < 0) return WCN_ERROR_INVALID_PARAMETERS;
  const int st = attn_kv_check(q, q_stride, k, v, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, head_dim,
                               max_seqlen_q, max_seqlen_k, softmax_scale, dtype);
  if (st != WCN_SUCCESS) return st;
  if (total_q > 0 && (!out || !lse || !aligned_to(out, 16))) return WCN_ERROR_INVALID_PARAMETERS;
  if (k_splits == 0) k_splits = wcn_attn_varlen_k_splits(num_seqs, max_seqlen_q, max_seqlen_k, heads, 0);
  const size_t need = wcn_attn_varlen_ksplit_workspace_bytes(total_q, total_k, heads, head_dim, 1, k_splits, 0);
  if (need > 0 && (!workspace || workspace_bytes < need || !aligned_to(workspace, 16))) return WCN_ERROR_INVALID_PARAMETERS;
  if (num_seqs == 0 || total_q == 0 || max_seqlen_q == 0) return WCN_SUCCESS;
  const AttnCall c{q, k, v, q_stride, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, max_seqlen_q, max_seqlen_k,
                   softmax_scale};
  // o [k_splits, total_q, heads, head_dim] first (a multiple of 64 bytes), ml [k_splits, total_q, heads, 2] after it
  float* o = (float*)workspace;
  const AttnKSplit ks{k_splits, total_q, o, o + (size_t)k_splits * (size_t)total_q * (size_t)heads * (size_t)head_dim};
  return attn_fwd_dispatch(c, head_dim, dtype, out, lse, variant, (hipStream_t)stream, ks);
}

int wcn_attn_varlen_kv_bwd(const void* dout, const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                           const void* out, const float* lse, const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs,
                           int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim, int32_t max_seqlen_q,
                           int32_t max_seqlen_k, float softmax_scale, int32_t dtype, void* dq, int64_t dq_stride, void* dk,
                           void* dv, int64_t dkv_stride, int32_t q_splits, void* workspace, size_t workspace_bytes,
                           wcn_stream_t stream) {
  return wcn_attn_varlen_kv_bwd_v(dout, q, q_stride, k, v, kv_stride, out, lse, cu_q, cu_k, num_seqs, total_q, total_k, heads,
                                  head_dim, max_seqlen_q, max_seqlen_k, softmax_scale, dtype, dq, dq_stride, dk, dv, dkv_stride,
                                  q_splits, workspace, workspace_bytes, WCN_ATTN_AUTO, stream);
}

int wcn_attn_varlen_kv_bwd_v(const void* dout, const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                             const void* out, const float* lse, const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs,
                             int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim, int32_t max_seqlen_q,
                             int32_t max_seqlen_k, float softmax_scale, int32_t dtype, void* dq, int64_t dq_stride, void* dk,
                             void* dv, int64_t dkv_stride, int32_t q_splits, void* workspace, size_t workspace_bytes,
                             int32_t variant, wcn_stream_t stream) {
  return wcn_attn_varlen_kv_bwd_s(dout, q, q_stride, k, v, kv_stride, out, lse, cu_q, cu_k, num_seqs, total_q, total_k, heads,
                                  head_dim, max_seqlen_q, max_seqlen_k, softmax_scale, dtype, dq, dq_stride, dk, dv, dkv_stride,
                                  q_splits, 1, workspace, workspace_bytes, variant, stream);
}

int wcn_attn_varlen_kv_bwd_s(const void* dout, const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                             const void* out, const float* lse, const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs,
                             int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim, int32_t max_seqlen_q,
                             int32_t max_seqlen_k, float softmax_scale, int32_t dtype, void* dq, int64_t dq_stride, void* dk,
                             void* dv, int64_t dkv_stride, int32_t q_splits, int32_t k_splits, void* workspace,
                             size_t workspace_bytes, int32_t variant, wcn_stream_t stream) {
  if (!attn_variant_ok(variant) || k_splits < 0) return WCN_ERROR_INVALID_PARAMETERS;
  const int st = attn_kv_check(q, q_stride, k, v, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, head_dim,
                               max_seqlen_q, max_seqlen_k, softmax_scale, dtype);
  if (st != WCN_SUCCESS) return st;
  const int64_t hd = (int64_t)heads * head_dim;
  if (q_splits < 0 || dq_stride < hd || dkv_stride < hd || (dq_stride & 7) || (dkv_stride & 7)) return WCN_ERROR_INVALID_PARAMETERS;
  if (total_q > 0 && (!dout || !out || !lse || !dq)) return WCN_ERROR_INVALID_PARAMETERS;
  if (total_k > 0 && (!dk || !dv)) return WCN_ERROR_INVALID_PARAMETERS;
  if (!aligned_to(dout, 16) || !aligned_to(out, 16) || !aligned_to(dq, 16) || !aligned_to(dk, 16) || !aligned_to(dv, 16) ||
      !aligned_to(workspace, 16))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (q_splits == 0) q_splits = wcn_attn_varlen_kv_splits(num_seqs, max_seqlen_q, max_seqlen_k, heads);
  if (k_splits == 0) k_splits = wcn_attn_varlen_k_splits(num_seqs, max_seqlen_q, max_seqlen_k, heads, 1);
  const size_t need = wcn_attn_varlen_ksplit_workspace_bytes(total_q, total_k, heads, head_dim, q_splits, k_splits, 1);
  if (workspace_bytes < need || (need > 0 && !workspace)) return WCN_ERROR_INVALID_PARAMETERS;
  if (num_seqs == 0 || (total_q == 0 && total_k == 0)) return WCN_SUCCESS;
  // the dK/dV partials come first, the dQ partials [k_splits, total_q, heads, head_dim] after them (both sizes are
  // multiples of 16 bytes, either may be empty), delta [total_q, heads] last
  const size_t dq_bytes = k_splits > 1 ? (size_t)k_splits * (size_t)total_q * (size_t)heads * (size_t)head_dim * sizeof(float) : 0;
  const size_t delta_bytes = (size_t)total_q * (size_t)heads * sizeof(float);
  float* part = (float*)workspace;
  float* delta = (float*)((char*)workspace + (need - delta_bytes));
  const AttnKSplit ks{k_splits, total_q, (float*)((char*)workspace + (need - delta_bytes - dq_bytes)), nullptr};
  const AttnCall c{q, k, v, q_stride, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, max_seqlen_q, max_seqlen_k,
                   softmax_scale};
  return attn_bwd_dispatch(c, head_dim, dtype, dout, out, lse, dq, dq_stride, dk, dv, dkv_stride, q_splits, part, delta,
                           variant, (hipStream_t)stream, ks);
}
