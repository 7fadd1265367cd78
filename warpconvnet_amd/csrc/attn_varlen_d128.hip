// attn_varlen_d128.hip - the varlen attention of attn_varlen.hip at head size 128 (the sparse DiT blocks at 1536 channels x
// 12 heads), on kernels with a work split of their own.  Same contract: separate Q / K / V row pointers with two strides and
// two boundary arrays, out / lse / dq / dk / dv as there, the empty-side conventions (out = 0, lse = -inf, dq = 0,
// dk = dv = 0), the exp2-domain online softmax, fixed summation order, no float atomics: two runs give the same bits.
//
// Why not the templates of attn_varlen.hip at D = 128: the accumulators and fragments of a wave double with the head size
// (dK/dV holds 161 VGPRs at D = 64), so one wave cannot own a whole head row at an occupancy worth having.
//
// The split.  A work item stays (sequence, 32-row block, head) - plus the split index in the split instantiations - and is
// run by a workgroup of TWO waves; wave w owns columns 64 w .. 64 w + 63 of the head.  It reads only that half of every
// Q / K / V / dO row (the global traffic of a wave is the D = 64 one-wave kernel's), keeps only that half's accumulators
// (two 32 x 32 blocks per output) and builds only its own transposed LDS image (64 x 36 elements, private to the wave).
//   score products   S^T = K Q^T (forward, dQ), S = Q K^T and dP = dO V^T (dK/dV), dP^T = V dO^T (dQ) reduce over all 128
//                    columns: each wave forms the partial over its 64 with a chain of four v_mfma_f32_32x32x16, writes the
//                    32 x 32 fp32 tile to LDS in lane-contiguous 16-byte pieces (piece g of lane l at float 4 (64 g + l):
//                    no bank conflict), and after ONE workgroup barrier adds its partner's tile: own + partner.  Float
//                    addition commutes, so both waves hold the same bits, and their softmax, their recomputed P and their dS
//                    are identical without further traffic.
//   exchange buffers two, alternated per tile ACROSS work items (the buffer index never resets): a tile written under
//                    barrier n is read before barrier n + 1 and its buffer is written again only after that barrier.  dQ
//                    and dK/dV exchange both of their tiles (S and dP) under the same barrier; dK/dV also stages the 32
//                    lse (wave 0) and delta (wave 1) values of the query block there.
//   output products  O^T += V^T P^T, dQ^T += K^T dS^T, dV^T += dO^T P, dK^T += Q^T dS need no exchange: the shared P / dS
//                    operand comes from the wave's own registers and multiplies the image of the wave's own columns; a wave
//                    stores its own 64 columns.  lse and the split forward's (m, l) are stored by wave 0.
// Loop bounds are uniform over the workgroup (one item, one split share), so a wave never skips a barrier; a block past its
// side's end exits for both waves together.  The transposed images are private to a wave: its LDS accesses complete in
// program order, and the barrier of every tile orders them as well.
// Split sweeps: q_splits (dK/dV) and k_splits (forward, dQ) with the shares, the fp32 partial layouts and the combine /
// reduce kernels of attn_varlen.h, instantiated at 128.  The shared-tile variant (WCN_ATTN_SHARED) is attn_varlen_d128_shared.hip;
// the entry points below choose between the two (wcn_attn_d128_variant).
// Resources (hipcc -Rpass-analysis=kernel-resource-usage --offload-arch=gfx950; bf16 and f16 alike; VGPRs + AGPRs, LDS
// per workgroup, waves per SIMD by registers, workgroups per CU by the 160 KiB of LDS):
//   forward          112 + 32   25 600 B   3 per SIMD   6 workgroups = 12 waves per CU: both limits agree
//   forward, split   108 + 32   25 600 B   3            6
//   dQ               144 + 32   41 984 B   2            3 workgroups = 6 waves per CU: LDS binds (1 KiB over a fourth)
//   dQ, split        139 + 32   41 984 B   2            3
//   dK/dV            176 + 64   51 712 B   2            3 workgroups = 6 waves per CU: LDS binds
//   dK/dV, split     164 + 64   51 712 B   2            3
//   delta 17, combine 28, reduce 22 VGPRs at D = 128, no LDS.
// None spills to scratch (ScratchSize 0, no VGPR or SGPR spill).  fp32 arithmetic of this file stays scalar (no packed
// fp32 instructions: see the Makefile).
#include "attn_varlen_d128.h"

namespace wcn {

// ---- forward --------------------------------------------------------------------------------------------------------
template <typename T, bool KSPLIT>
__global__ __launch_bounds__(kPairThreads) void attn_pair_fwd_kernel(const AttnOperands<T> a, int64_t items, int nblk, float c2,
                                                                     T* __restrict__ out, float* __restrict__ lse,
                                                                     const AttnKSplit ks) {
  typedef typename AFrag<T>::type frag;
  constexpr int D = 128, NS = kPairCols / 16, NMB = kPairCols / 32;
  __shared__ __attribute__((aligned(16))) T vt_all[2][kPairTr];
  __shared__ __attribute__((aligned(16))) float xs[2][2][kPairTile];  // [buffer][wave]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int col0 = kPairCols * wave;
  T* vt = vt_all[wave];
  const int heads = a.heads;
  const int64_t qp = a.q_stride, kp = a.kv_stride;
  int cur = 0;
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
    if (w.b0 >= w.len_q) continue;  // (the same for both waves)
    int k_end = w.len_k;
    if (KSPLIT) attn_key_share(w.len_k, ks.k_splits, split, k_beg, k_end);
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D + col0;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D + col0;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D + col0;
    frag qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = load8<T>(q, qp, w.b0 + r, w.len_q, 16 * s + 8 * h);
    a_f32x16 acc[NMB];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mb][i] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int k0 = k_beg; k0 < k_end; k0 += kAttnTile, cur ^= 1) {
      a_f32x16 st;
      frag vf[NS];
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        st = AFrag<T>::mfma(load8<T>(k, kp, k0 + r, w.len_k, 16 * s + 8 * h), qf[s], st);
        vf[s] = load8<T>(v, kp, k0 + r, w.len_k, 16 * s + 8 * h);
      }
      put_tile(xs[cur][wave], st, lane);
      stage_frags<T, kPairCols>(vt, vf, r, h);
      __syncthreads();  // both partial tiles are written, the image is staged
      add_tile(st, xs[cur][wave ^ 1], lane);
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
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const frag pf = acc_frag<T>(x, s);
#pragma unroll
        for (int mb = 0; mb < NMB; ++mb) acc[mb] = AFrag<T>::mfma(read_tr<T>(vt, mb, s, r, h), pf, acc[mb]);
      }
    }
    const int row = w.b0 + r;
    if (row >= w.len_q) continue;  // (stores only: no barrier follows in this item)
    if (KSPLIT) {
      // the share's state as it stands: an empty share leaves m = -inf, l = 0 and a zero accumulator
      const int64_t idx = ((int64_t)split * ks.total_q + w.beg_q + row) * heads + w.hd;
      store_dcol_f32<kPairCols>(ks.o + idx * D + col0, acc, h);
      if (wave == 0 && h == 0) *reinterpret_cast<float2*>(ks.ml + 2 * idx) = make_float2(m, l);
    } else {
      // no key: the accumulator is still zero and is stored as exact zeros, lse = -inf
      const bool any = w.len_k > 0;
      const int64_t t = w.beg_q + row;
      store_dcol<T, kPairCols>(out + (t * heads + w.hd) * D + col0, acc, any ? 1.f / l : 0.f, h);
      if (wave == 0 && h == 0) lse[t * heads + w.hd] = any ? (m + __log2f(l)) * kLn2 : -INFINITY;
    }
  }
}

// ---- dK, dV ---------------------------------------------------------------------------------------------------------
// One (sequence, 32-key block, head) - or, with SPLIT, one share of its query blocks, unscaled fp32 sums to
// part [q_splits, total_k, 2, H, 128] - as attn_bwd_dkdv_kernel, each wave on its 64 columns of K, V, Q, dO, dK and dV.
template <typename T, bool SPLIT>
__global__ __launch_bounds__(kPairThreads) void attn_pair_dkdv_kernel(const AttnOperands<T> a, const T* __restrict__ dout,
                                                                      const float* __restrict__ lse,
                                                                      const float* __restrict__ delta, int64_t items, int nblk,
                                                                      float c2, float scale, T* __restrict__ dk_out,
                                                                      T* __restrict__ dv_out, int64_t dkv_stride, int q_splits,
                                                                      int64_t total_k, float* __restrict__ part) {
  typedef typename AFrag<T>::type frag;
  constexpr int D = 128, NS = kPairCols / 16, NMB = kPairCols / 32;
  __shared__ __attribute__((aligned(16))) T qt_all[2][kPairTr];
  __shared__ __attribute__((aligned(16))) T dot_all[2][kPairTr];
  __shared__ __attribute__((aligned(16))) float xs[2][2][2][kPairTile];  // [buffer][wave][S, dP]
  __shared__ __attribute__((aligned(16))) float s_lse[2][kAttnTile];     // [buffer]
  __shared__ __attribute__((aligned(16))) float s_del[2][kAttnTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int col0 = kPairCols * wave;
  T* qt = qt_all[wave];
  T* dot = dot_all[wave];
  const int heads = a.heads;
  const int64_t qp = a.q_stride, kp = a.kv_stride, opitch = (int64_t)heads * D;
  int cur = 0;
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
    if (w.b0 >= w.len_k) continue;  // (the same for both waves)
    // the query rows this item sweeps: all of them, or split's share of the 32-row blocks (an empty share stores zeros)
    int q_beg = 0, q_end = w.len_q;
    if (SPLIT) attn_key_share(w.len_q, q_splits, split, q_beg, q_end);
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D + col0;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D + col0;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D + col0;
    const T* dO = dout + w.beg_q * opitch + (int64_t)w.hd * D + col0;
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
    for (int q0 = q_beg; q0 < q_end; q0 += kAttnTile, cur ^= 1) {
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
      put_tile(xs[cur][wave][0], sc, lane);
      put_tile(xs[cur][wave][1], dp, lane);
      stage_frags<T, kPairCols>(qt, qf, r, h);
      stage_frags<T, kPairCols>(dot, df, r, h);
      if (h == 0) {
        // this sequence has a key (b0 < len_k), so the forward's lse of its queries is finite; the test keeps an lse of
        // -inf (a caller's own buffer) out of the subtraction below all the same
        const int qr = q0 + r;
        const bool ok = qr < w.len_q;
        const int64_t t = w.beg_q + qr;
        if (wave == 0) {
          const float L = ok ? lse[t * heads + w.hd] : 0.f;
          s_lse[cur][r] = L > -INFINITY ? L * kLog2e : INFINITY;  // +inf: p = exp2(-inf) = 0
        } else {
          s_del[cur][r] = ok ? delta[t * heads + w.hd] : 0.f;
        }
      }
      __syncthreads();  // the partial tiles, lse and delta of this query block are written, the images are staged
      add_tile(sc, xs[cur][wave ^ 1][0], lane);
      add_tile(dp, xs[cur][wave ^ 1][1], lane);
      // Rows of sc / dp are queries, the lane's column is its key.  Query rows past len_q carry Q = dO = 0, lse =
      // delta = 0: p = 1, dS = 0, and their dO^T / Q^T columns are zero, so they add nothing.  Keys past len_k: p = 0.
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
          dv[mb] = AFrag<T>::mfma(read_tr<T>(dot, mb, s, r, h), pf, dv[mb]);
          dk[mb] = AFrag<T>::mfma(read_tr<T>(qt, mb, s, r, h), dsf, dk[mb]);
        }
      }
    }
    if (key >= w.len_k) continue;  // (stores only: no barrier follows in this item)
    if (SPLIT) {
      float* dst = part + (((int64_t)split * total_k + w.beg_k + key) * 2 * heads + w.hd) * D + col0;
      store_dcol_f32<kPairCols>(dst, dk, h);
      store_dcol_f32<kPairCols>(dst + (int64_t)heads * D, dv, h);
    } else {
      const int64_t off = (w.beg_k + key) * dkv_stride + (int64_t)w.hd * D + col0;
      store_dcol<T, kPairCols>(dk_out + off, dk, scale, h);
      store_dcol<T, kPairCols>(dv_out + off, dv, 1.f, h);
    }
  }
}

// ---- dQ -------------------------------------------------------------------------------------------------------------
// One (sequence, 32-query block, head) - or, with KSPLIT, one share of its keys, unscaled fp32 dq to ks.o - as
// attn_bwd_dq_kernel, each wave on its 64 columns of Q, dO, K, V and dQ.
template <typename T, bool KSPLIT>
__global__ __launch_bounds__(kPairThreads) void attn_pair_dq_kernel(const AttnOperands<T> a, const T* __restrict__ dout,
                                                                    const float* __restrict__ lse,
                                                                    const float* __restrict__ delta, int64_t items, int nblk,
                                                                    float c2, float scale, T* __restrict__ dq_out,
                                                                    int64_t dq_stride, const AttnKSplit ks) {
  typedef typename AFrag<T>::type frag;
  constexpr int D = 128, NS = kPairCols / 16, NMB = kPairCols / 32;
  __shared__ __attribute__((aligned(16))) T kt_all[2][kPairTr];
  __shared__ __attribute__((aligned(16))) float xs[2][2][2][kPairTile];  // [buffer][wave][S^T, dP^T]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int col0 = kPairCols * wave;
  T* kt = kt_all[wave];
  const int heads = a.heads;
  const int64_t qp = a.q_stride, kp = a.kv_stride, opitch = (int64_t)heads * D;
  int cur = 0;
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
    if (w.b0 >= w.len_q) continue;  // (the same for both waves)
    int k_end = w.len_k;
    if (KSPLIT) attn_key_share(w.len_k, ks.k_splits, split, k_beg, k_end);
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D + col0;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D + col0;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D + col0;
    const T* dO = dout + w.beg_q * opitch + (int64_t)w.hd * D + col0;
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
    for (int k0 = k_beg; k0 < k_end; k0 += kAttnTile, cur ^= 1) {
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
      put_tile(xs[cur][wave][0], st, lane);
      put_tile(xs[cur][wave][1], dpt, lane);
      stage_frags<T, kPairCols>(kt, kf, r, h);
      __syncthreads();  // both waves' partial tiles are written, the image is staged
      add_tile(st, xs[cur][wave ^ 1][0], lane);
      add_tile(dpt, xs[cur][wave ^ 1][1], lane);
      // rows are keys, the lane's column its query; keys past len_k get p = 0 (their K, V rows were read as zeros)
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
        for (int mb = 0; mb < NMB; ++mb) dq[mb] = AFrag<T>::mfma(read_tr<T>(kt, mb, s, r, h), dsf, dq[mb]);
      }
    }
    if (!ok) continue;  // (stores only: no barrier follows in this item)
    if (KSPLIT)
      store_dcol_f32<kPairCols>(ks.o + (((int64_t)split * ks.total_q + w.beg_q + row) * heads + w.hd) * D + col0, dq, h);
    else
      store_dcol<T, kPairCols>(dq_out + (w.beg_q + row) * dq_stride + (int64_t)w.hd * D + col0, dq, scale, h);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
static inline int pair_blocks(int max_seqlen) { return (max_seqlen + kAttnTile - 1) / kAttnTile; }

// k_splits > 1: the split-key kernel into the partials `ks`, then the combine; 1: the unsplit kernel.
template <typename T>
static int attn_pair_fwd_t(const AttnCall& c, void* out, float* lse, const AttnKSplit& ks, hipStream_t s) {
  constexpr int D = 128;
  const int nblk = pair_blocks(c.max_q);
  const int64_t items = c.num_seqs * nblk * c.heads * ks.k_splits;
  const AttnOperands<T> a = attn_operands<T>(c);
  const float c2 = c.scale * kLog2e;
  const dim3 wg(kPairThreads);
  if (items > 0) {
    if (ks.k_splits > 1) {
      hipLaunchKernelGGL((attn_pair_fwd_kernel<T, true>), dim3(pair_grid(items)), wg, 0, s, a, items, nblk, c2, (T*)out, lse, ks);
      const int64_t n = c.total_q * c.heads * (D / 4);
      hipLaunchKernelGGL((attn_fwd_combine_kernel<T, D>), dim3(pair_grid((n + 255) / 256)), dim3(256), 0, s, ks, c.cu_q,
                         c.num_seqs, c.heads, (T*)out, lse);
    } else {
      hipLaunchKernelGGL((attn_pair_fwd_kernel<T, false>), dim3(pair_grid(items)), wg, 0, s, a, items, nblk, c2, (T*)out, lse, ks);
    }
  }
  return hipGetLastError() == hipSuccess ? WCN_SUCCESS : WCN_ERROR_KERNEL_EXECUTION;
}

template <typename T>
static int attn_pair_bwd_t(const AttnCall& c, const void* dout, const void* out, const float* lse, void* dq, int64_t dq_stride,
                           void* dk, void* dv, int64_t dkv_stride, int q_splits, float* part, float* delta, const AttnKSplit& ks,
                           hipStream_t s) {
  constexpr int D = 128;
  const AttnOperands<T> a = attn_operands<T>(c);
  const float c2 = c.scale * kLog2e;
  const int64_t rows = c.total_q * c.heads;
  const int nblk_q = pair_blocks(c.max_q), nblk_k = pair_blocks(c.max_k);
  const int64_t items_q = c.num_seqs * nblk_q * c.heads, items_k = c.num_seqs * nblk_k * c.heads;
  const dim3 wg(kPairThreads);
  if (rows > 0)
    hipLaunchKernelGGL((attn_delta_kernel<T, D>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, (const T*)dout,
                       (const T*)out, rows, delta);
  if (items_k > 0 && c.total_k > 0) {
    if (q_splits > 1) {
      hipLaunchKernelGGL((attn_pair_dkdv_kernel<T, true>), dim3(pair_grid(items_k * q_splits)), wg, 0, s, a, (const T*)dout, lse,
                         (const float*)delta, items_k * q_splits, nblk_k, c2, c.scale, (T*)dk, (T*)dv, dkv_stride, q_splits,
                         c.total_k, part);
      const int64_t n = c.total_k * 2 * c.heads * (D / 4);
      hipLaunchKernelGGL((attn_dkdv_reduce_kernel<T, D>), dim3(pair_grid((n + 255) / 256)), dim3(256), 0, s, (const float*)part,
                         c.cu_k, c.num_seqs, c.total_k, c.heads, q_splits, c.scale, (T*)dk, (T*)dv, dkv_stride);
    } else {
      hipLaunchKernelGGL((attn_pair_dkdv_kernel<T, false>), dim3(pair_grid(items_k)), wg, 0, s, a, (const T*)dout, lse,
                         (const float*)delta, items_k, nblk_k, c2, c.scale, (T*)dk, (T*)dv, dkv_stride, 1, c.total_k,
                         (float*)nullptr);
    }
  }
  if (items_q > 0 && c.total_q > 0) {
    if (ks.k_splits > 1) {
      const int64_t items = items_q * ks.k_splits;
      hipLaunchKernelGGL((attn_pair_dq_kernel<T, true>), dim3(pair_grid(items)), wg, 0, s, a, (const T*)dout, lse,
                         (const float*)delta, items, nblk_q, c2, c.scale, (T*)dq, dq_stride, ks);
      const int64_t n = c.total_q * c.heads * (D / 4);
      hipLaunchKernelGGL((attn_dq_reduce_kernel<T, D>), dim3(pair_grid((n + 255) / 256)), dim3(256), 0, s, ks, c.cu_q, c.num_seqs,
                         c.heads, c.scale, (T*)dq, dq_stride);
    } else {
      hipLaunchKernelGGL((attn_pair_dq_kernel<T, false>), dim3(pair_grid(items_q)), wg, 0, s, a, (const T*)dout, lse,
                         (const float*)delta, items_q, nblk_q, c2, c.scale, (T*)dq, dq_stride, ks);
    }
  }
  return hipGetLastError() == hipSuccess ? WCN_SUCCESS : WCN_ERROR_KERNEL_EXECUTION;
}

}  // namespace wcn

using namespace wcn;

int wcn_attn_d128_supported(int32_t head_dim, int32_t dtype) {
  return head_dim == 128 && (dtype == WCN_F16 || dtype == WCN_BF16) ? 1 : 0;
}

// What WCN_ATTN_AUTO resolves to at this head size: the shared-tile kernels from the shortest measured swept length at which
// they were ahead of the pair kernels in both directions by more than the spread of the rounds (8 192 rows;
// at 2 048 the forward + backward lead of 2 % is inside the spread), the pair kernels below it.
constexpr int32_t kD128SharedMinSweep = 8192;
static bool d128_variant_ok(int32_t v) { return v == WCN_ATTN_AUTO || v == WCN_ATTN_ONE_WAVE || v == WCN_ATTN_SHARED; }

int32_t wcn_attn_d128_variant(int64_t num_seqs, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t heads, int32_t direction) {
  if (num_seqs < 1 || max_seqlen_q < 1 || max_seqlen_k < 1 || heads < 1) return WCN_ATTN_ONE_WAVE;
  const int32_t sweep = direction == 0 ? max_seqlen_k : (max_seqlen_q > max_seqlen_k ? max_seqlen_q : max_seqlen_k);
  return sweep >= kD128SharedMinSweep ? WCN_ATTN_SHARED : WCN_ATTN_ONE_WAVE;
}

int wcn_attn_d128_fwd(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride, const int32_t* cu_q,
                      const int32_t* cu_k, int64_t num_seqs, int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim,
                      int32_t max_seqlen_q, int32_t max_seqlen_k, float softmax_scale, int32_t dtype, void* out, float* lse,
                      int32_t k_splits, void* workspace, size_t workspace_bytes, wcn_stream_t stream) {
  return wcn_attn_d128_fwd_v(q, q_stride, k, v, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, head_dim, max_seqlen_q,
                             max_seqlen_k, softmax_scale, dtype, out, lse, k_splits, workspace, workspace_bytes, WCN_ATTN_AUTO,
                             stream);
}

int wcn_attn_d128_fwd_v(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride, const int32_t* cu_q,
                        const int32_t* cu_k, int64_t num_seqs, int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim,
                        int32_t max_seqlen_q, int32_t max_seqlen_k, float softmax_scale, int32_t dtype, void* out, float* lse,
                        int32_t k_splits, void* workspace, size_t workspace_bytes, int32_t variant, wcn_stream_t stream) {
  if (!d128_variant_ok(variant) || k_splits < 0) return WCN_ERROR_INVALID_PARAMETERS;
  const int st = attn_kv_check(q, q_stride, k, v, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, head_dim,
                               max_seqlen_q, max_seqlen_k, softmax_scale, wcn_attn_d128_supported(head_dim, dtype));
  if (st != WCN_SUCCESS) return st;
  if (total_q > 0 && (!out || !lse || !aligned_to(out, 16))) return WCN_ERROR_INVALID_PARAMETERS;
  if (k_splits == 0) k_splits = wcn_attn_varlen_k_splits(num_seqs, max_seqlen_q, max_seqlen_k, heads, 0);
  const size_t need = wcn_attn_varlen_ksplit_workspace_bytes(total_q, total_k, heads, head_dim, 1, k_splits, 0);
  if (need > 0 && (!workspace || workspace_bytes < need || !aligned_to(workspace, 16))) return WCN_ERROR_INVALID_PARAMETERS;
  if (num_seqs == 0 || total_q == 0 || max_seqlen_q == 0) return WCN_SUCCESS;
  const AttnCall c{q, k, v, q_stride, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, max_seqlen_q, max_seqlen_k,
                   softmax_scale};
  // o [k_splits, total_q, heads, 128] first, ml [k_splits, total_q, heads, 2] after it (the layout of the narrower heads)
  float* o = (float*)workspace;
  const AttnKSplit ks{k_splits, total_q, o, o + (size_t)k_splits * (size_t)total_q * (size_t)heads * (size_t)head_dim};
  if (variant == WCN_ATTN_AUTO) variant = wcn_attn_d128_variant(num_seqs, max_seqlen_q, max_seqlen_k, heads, 0);
  if (variant == WCN_ATTN_SHARED) return attn_wg_fwd(dtype, c, out, lse, ks, (hipStream_t)stream);
  return with_dtype16(dtype, [&](auto t) { return attn_pair_fwd_t<decltype(t)>(c, out, lse, ks, (hipStream_t)stream); });
}

int wcn_attn_d128_bwd(const void* dout, const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                      const void* out, const float* lse, const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs,
                      int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim, int32_t max_seqlen_q,
                      int32_t max_seqlen_k, float softmax_scale, int32_t dtype, void* dq, int64_t dq_stride, void* dk, void* dv,
                      int64_t dkv_stride, int32_t q_splits, int32_t k_splits, void* workspace, size_t workspace_bytes,
                      wcn_stream_t stream) {
  return wcn_attn_d128_bwd_v(dout, q, q_stride, k, v, kv_stride, out, lse, cu_q, cu_k, num_seqs, total_q, total_k, heads, head_dim,
                             max_seqlen_q, max_seqlen_k, softmax_scale, dtype, dq, dq_stride, dk, dv, dkv_stride, q_splits, k_splits,
                             workspace, workspace_bytes, WCN_ATTN_AUTO, stream);
}

int wcn_attn_d128_bwd_v(const void* dout, const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                        const void* out, const float* lse, const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs,
                        int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim, int32_t max_seqlen_q,
                        int32_t max_seqlen_k, float softmax_scale, int32_t dtype, void* dq, int64_t dq_stride, void* dk, void* dv,
                        int64_t dkv_stride, int32_t q_splits, int32_t k_splits, void* workspace, size_t workspace_bytes,
                        int32_t variant, wcn_stream_t stream) {
  if (!d128_variant_ok(variant) || k_splits < 0 || q_splits < 0) return WCN_ERROR_INVALID_PARAMETERS;
  const int st = attn_kv_check(q, q_stride, k, v, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, head_dim,
                               max_seqlen_q, max_seqlen_k, softmax_scale, wcn_attn_d128_supported(head_dim, dtype));
  if (st != WCN_SUCCESS) return st;
  const int64_t hd = (int64_t)heads * head_dim;
  if (dq_stride < hd || dkv_stride < hd || (dq_stride & 7) || (dkv_stride & 7)) return WCN_ERROR_INVALID_PARAMETERS;
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
  // the dK/dV partials first, the dQ partials [k_splits, total_q, heads, 128] after them (either may be empty), delta
  // [total_q, heads] last: the layout of wcn_attn_varlen_kv_bwd_s
  const size_t dq_bytes = k_splits > 1 ? (size_t)k_splits * (size_t)total_q * (size_t)heads * (size_t)head_dim * sizeof(float) : 0;
  const size_t delta_bytes = (size_t)total_q * (size_t)heads * sizeof(float);
  float* part = (float*)workspace;
  float* delta = (float*)((char*)workspace + (need - delta_bytes));
  const AttnKSplit ks{k_splits, total_q, (float*)((char*)workspace + (need - delta_bytes - dq_bytes)), nullptr};
  const AttnCall c{q, k, v, q_stride, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, max_seqlen_q, max_seqlen_k,
                   softmax_scale};
  if (variant == WCN_ATTN_AUTO) variant = wcn_attn_d128_variant(num_seqs, max_seqlen_q, max_seqlen_k, heads, 1);
  if (variant == WCN_ATTN_SHARED)
    return attn_wg_bwd(dtype, c, dout, out, lse, dq, dq_stride, dk, dv, dkv_stride, q_splits, part, delta, ks, (hipStream_t)stream);
  return with_dtype16(dtype, [&](auto t) {
    return attn_pair_bwd_t<decltype(t)>(c, dout, out, lse, dq, dq_stride, dk, dv, dkv_stride, q_splits, part, delta, ks,
                                        (hipStream_t)stream);
  });
}
