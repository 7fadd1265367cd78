// attn_varlen_d128_shared.hip - the shared-tile variant (WCN_ATTN_SHARED) of the head-size-128 attention of
// attn_varlen_d128.hip: same contract, same bits.  In the pair kernels every wave pair fetches every tile of the swept side
// from global memory itself; here a workgroup of P pairs stages each tile once.
//
// The split.  A work item is (sequence, 32 P-row block, head [, split share]) run by 2 P waves.  Pair p = wave >> 1 owns rows
// b0 + 32 p .. + 31 of the block, wave w = wave & 1 of a pair owns columns 64 w .. 64 w + 63 of the head, as in the pair
// kernels.  A pair whose rows lie past the side's end computes on zero rows, stages its pieces, reaches every barrier and
// stores nothing.
// Staging.  A 32 x 128 tile of the swept side is 512 pieces of 16 bytes; thread tid owns pieces tid + 128 P j (one at P = 4,
// two at P = 2).  They go to LDS in the layouts the pair kernels read: a row-major image (pitch 136 elements: what load8
// returns for a row and 8 columns) for the A operand of the score products, and the two per-column-half transposed images
// (64 x kAttnPitch each) for the output products.  Forward: K rows, V^T.  dQ: K rows, V rows, K^T.  dK/dV: Q rows, dO rows,
// Q^T, dO^T and the block's 32 lse (threads 0..31) and 32 delta (threads 32..63) values.  Global loads of a later tile are
// issued before the barrier and the MFMAs of the current one and written to LDS after them.
// Arithmetic.  Every wave issues the pair kernel's instructions on its rows and columns: the same tile order, the same chain of
// four MFMAs per partial (operand values from LDS instead of global memory, zeros past a sequence end either way), put_tile /
// add_tile own + partner, the same masks, exp2-domain softmax, stores, split shares and partial layouts, and the combine /
// reduce / delta kernels of attn_varlen.h.  out, lse, dq, dk, dv carry the pair kernels' bits
// (tests/test_gpu_attention_d128_shared.py).  No float atomics; the host never reads cu_*.
//
// Schedule (XB = 2 exchange buffers: ONE barrier per tile).  All images are double buffers, buffer = tile index & 1 within the
// item.  Prologue: rows of tiles 0 and 1 and the transposed images (and lse / delta) of tile 0 are staged; barrier A; every
// wave forms its partial of tile 0 and puts it.  Phase t = one loop trip: [loads of the rows of tile t + 2 and the images of
// tile t + 1 are issued]; barrier t; add the partner's partial of tile t, softmax / dS, the output MFMAs of tile t; form and
// put the partial of tile t + 1; write the images of tile t + 1 and the rows of tile t + 2.  A barrier E ends the item.
// Hazards - every LDS write against the reads before and after it:
//   partial of tile t + 1 -> xs[(t+1)&1]: written in phase t; last read (tile t - 1) in phase t - 1, before barrier t; next
//                      read in phase t + 1, after barrier t + 1.
//   rows of tile t + 2 -> rows[t&1]: written in phase t; last read (the partial of tile t) in phase t - 1 (or after barrier A),
//                      before barrier t; next read in phase t + 1, after barrier t + 1.  Phase t itself reads rows[(t+1)&1].
//   images, lse / delta of tile t + 1 -> img[(t+1)&1]: written in phase t; last read (tile t - 1) in phase t - 1, before
//                      barrier t; next read in phase t + 1, after barrier t + 1.  Phase t itself reads img[t&1].
//   prologue writes (rows[0], rows[1], img[0]; xs[0] after barrier A): every read of the previous item is before its barrier E.
// XB = 1 (dQ: two exchanged tiles per wave, and 8 waves would need 128 KiB of exchange): one buffer and a SECOND barrier per
// tile in front of the put of tile t + 1, which separates it from the partner's read of tile t in the same phase; the read of
// tile t + 1 is after barrier t + 1 as before.
// Barriers.  Loop bounds are uniform over the workgroup (one sequence, one split share); the only `continue` in front of a
// barrier tests the block's first row b0, the same for all 2 P waves; an empty sweep skips barriers A .. E for all of them; the
// store guards come after barrier E.  No wave leaves an item while another one of its workgroup can still reach a barrier.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage --offload-arch=gfx950; bf16 and f16 alike; VGPRs + AGPRs, LDS per
// workgroup, workgroups per CU by the 160 KiB of LDS):
//   forward          P = 4, XB = 2   147 + 0    101 376 B   1 workgroup = 8 waves per CU
//   forward, split   P = 4, XB = 2   137 + 0    101 376 B   1
//   dQ               P = 4, XB = 1   177 + 0    118 784 B   1 workgroup = 8 waves per CU
//   dQ, split        P = 4, XB = 1   172 + 0    118 784 B   1
//   dK/dV            P = 2, XB = 2   216 + 96   137 728 B   1 workgroup = 4 waves per CU
//   dK/dV, split     P = 2, XB = 2   186 + 96   137 728 B   1
// dK/dV at P = 4, XB = 1 needs the same LDS but 256 VGPRs and spills 8 of them in the unsplit instantiation, so it runs at
// P = 2.  None of the six spills to scratch (ScratchSize 0, no VGPR or SGPR spill).  fp32 arithmetic of this file stays scalar
// (no packed fp32 instructions: see the Makefile) - bit identity with the pair kernels depends on it.
#include "attn_varlen_d128.h"

namespace wcn {

// ---- shared-tile variants: P wave pairs per workgroup, every tile of the swept side staged once in LDS --------------------
// (the header comment has the split, the schedule and the hazard argument)
constexpr int kWgRowPitch = 128 + 8;                  // row-major image of a 32 x 128 tile: 16-B aligned rows, elements
constexpr int kWgRows = kAttnTile * kWgRowPitch;      // elements of a row-major image
constexpr int kWgTr = 2 * kPairTr;                    // elements of the two transposed images (columns 0..63, 64..127)
constexpr int kWgPieces = kAttnTile * 128 / 8;        // 16-byte pieces of a tile

// Piece c of a tile is (row c & 31, d-chunk c >> 5): thread tid of a workgroup of 512 / NPC threads owns pieces
// tid + (512 / NPC) j.  Rows past the sequence end are zeros, as load8 returns them.
template <typename T, int NPC>
__device__ __forceinline__ void load_pieces(typename AFrag<T>::type* v, const T* __restrict__ base, int64_t pitch, int row0,
                                            int len, int tid) {
#pragma unroll
  for (int j = 0; j < NPC; ++j) {
    const int c = tid + (kWgPieces / NPC) * j;
    v[j] = load8<T>(base, pitch, row0 + (c & 31), len, 8 * (c >> 5));
  }
}
template <typename T, int NPC>
__device__ __forceinline__ void put_row_pieces(T* __restrict__ rows, const typename AFrag<T>::type* v, int tid) {
#pragma unroll
  for (int j = 0; j < NPC; ++j) {
    const int c = tid + (kWgPieces / NPC) * j;
    *reinterpret_cast<typename AFrag<T>::type*>(rows + (c & 31) * kWgRowPitch + 8 * (c >> 5)) = v[j];
  }
}
// d-chunks 0..7 land in the image of columns 0..63, 8..15 in the one of columns 64..127 (kPairTr = 64 kAttnPitch apart).
template <typename T, int NPC>
__device__ __forceinline__ void put_tr_pieces(T* __restrict__ img, const typename AFrag<T>::type* v, int tid) {
#pragma unroll
  for (int j = 0; j < NPC; ++j) {
    const int c = tid + (kWgPieces / NPC) * j;
#pragma unroll
    for (int e = 0; e < 8; ++e) img[(8 * (c >> 5) + e) * kAttnPitch + (c & 31)] = v[j][e];
  }
}
// A wave's partial score tile over its 64 columns: the pair kernels' chain of four MFMAs, the A operand (what load8 returns
// for row r, columns col0 + 16 s + 8 h .. + 7) read from a row-major image.
template <typename T>
__device__ __forceinline__ a_f32x16 rows_times(const T* __restrict__ rows, const typename AFrag<T>::type* b, int r, int h,
                                               int col0) {
  a_f32x16 t;
#pragma unroll
  for (int i = 0; i < 16; ++i) t[i] = 0.f;
#pragma unroll
  for (int s = 0; s < kPairCols / 16; ++s)
    t = AFrag<T>::mfma(*reinterpret_cast<const typename AFrag<T>::type*>(rows + r * kWgRowPitch + col0 + 16 * s + 8 * h), b[s], t);
  return t;
}

// Forward of one (sequence, 32 P-query block, head [, key share]): K rows and the V^T images staged once per key tile.
template <typename T, int P, int XB, bool KSPLIT>
__global__ __launch_bounds__(128 * P) void attn_wg_fwd_kernel(const AttnOperands<T> a, int64_t items, int nblk, float c2,
                                                              T* __restrict__ out, float* __restrict__ lse,
                                                              const AttnKSplit ks) {
  typedef typename AFrag<T>::type frag;
  constexpr int D = 128, NS = kPairCols / 16, NMB = kPairCols / 32, NPC = 4 / P;
  __shared__ __attribute__((aligned(16))) T kr[2][kWgRows];
  __shared__ __attribute__((aligned(16))) T vt[2][kWgTr];
  __shared__ __attribute__((aligned(16))) float xs[XB][2 * P][kPairTile];  // [buffer][wave]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int col0 = kPairCols * (wave & 1);
  const int heads = a.heads;
  const int64_t qp = a.q_stride, kp = a.kv_stride;
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    AttnItem w;
    int split = 0, k_beg = 0;
    if (KSPLIT) {
      const int64_t t = id / heads;
      split = (int)(t % ks.k_splits);
      attn_item((t / ks.k_splits) * heads + id % heads, nblk, heads, a.cu_q, a.cu_k, w, kAttnTile * P);
    } else {
      attn_item(id, nblk, heads, a.cu_q, a.cu_k, w, kAttnTile * P);
    }
    if (w.b0 >= w.len_q) continue;  // (the same for every wave of the workgroup: no barrier is passed by)
    int k_end = w.len_k;
    if (KSPLIT) attn_key_share(w.len_k, ks.k_splits, split, k_beg, k_end);
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D + col0;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D;
    const int rb = w.b0 + kAttnTile * (wave >> 1);  // this pair's rows; past the end they are zeros and nothing is stored
    frag qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = load8<T>(q, qp, rb + r, w.len_q, 16 * s + 8 * h);
    a_f32x16 acc[NMB];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mb][i] = 0.f;
    float m = -INFINITY, l = 0.f;
    if (k_beg < k_end) {  // (uniform: one sequence, one share)
      frag kn[NPC], vn[NPC];
      load_pieces<T, NPC>(kn, k, kp, k_beg, w.len_k, tid);
      load_pieces<T, NPC>(vn, v, kp, k_beg, w.len_k, tid);
      put_row_pieces<T, NPC>(kr[0], kn, tid);
      put_tr_pieces<T, NPC>(vt[0], vn, tid);
      if (k_beg + kAttnTile < k_end) {
        load_pieces<T, NPC>(kn, k, kp, k_beg + kAttnTile, w.len_k, tid);
        put_row_pieces<T, NPC>(kr[1], kn, tid);
      }
      __syncthreads();  // tiles 0 and 1 are staged
      a_f32x16 st = rows_times<T>(kr[0], qf, r, h, col0);
      put_tile(xs[0][wave], st, lane);
      for (int k0 = k_beg, cur = 0; k0 < k_end; k0 += kAttnTile, cur ^= 1) {
        const bool more1 = k0 + kAttnTile < k_end, more2 = k0 + 2 * kAttnTile < k_end;
        if (more2) load_pieces<T, NPC>(kn, k, kp, k0 + 2 * kAttnTile, w.len_k, tid);  // in flight during this tile's MFMAs
        if (more1) load_pieces<T, NPC>(vn, v, kp, k0 + kAttnTile, w.len_k, tid);
        __syncthreads();  // this tile's partials and images are written
        add_tile(st, xs[XB == 2 ? cur : 0][wave ^ 1], lane);
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
        const T* img = vt[cur] + kPairTr * (wave & 1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const frag pf = acc_frag<T>(x, s);
#pragma unroll
          for (int mb = 0; mb < NMB; ++mb) acc[mb] = AFrag<T>::mfma(read_tr<T>(img, mb, s, r, h), pf, acc[mb]);
        }
        if (more1) {
          if (XB == 1) __syncthreads();  // the one exchange buffer has been read by every partner
          st = rows_times<T>(kr[cur ^ 1], qf, r, h, col0);
          put_tile(xs[XB == 2 ? cur ^ 1 : 0][wave], st, lane);
          put_tr_pieces<T, NPC>(vt[cur ^ 1], vn, tid);
        }
        if (more2) put_row_pieces<T, NPC>(kr[cur], kn, tid);
      }
      __syncthreads();  // the last tile's reads are done before the next item stages its first
    }
    const int row = rb + r;
    if (row >= w.len_q) continue;  // (stores only: no barrier follows in this item)
    if (KSPLIT) {
      const int64_t idx = ((int64_t)split * ks.total_q + w.beg_q + row) * heads + w.hd;
      store_dcol_f32<kPairCols>(ks.o + idx * D + col0, acc, h);
      if ((wave & 1) == 0 && h == 0) *reinterpret_cast<float2*>(ks.ml + 2 * idx) = make_float2(m, l);
    } else {
      const bool any = w.len_k > 0;
      const int64_t t = w.beg_q + row;
      store_dcol<T, kPairCols>(out + (t * heads + w.hd) * D + col0, acc, any ? 1.f / l : 0.f, h);
      if ((wave & 1) == 0 && h == 0) lse[t * heads + w.hd] = any ? (m + __log2f(l)) * kLn2 : -INFINITY;
    }
  }
}

// dQ of one (sequence, 32 P-query block, head [, key share]): K rows, V rows and the K^T images staged once per key tile.
// The K pieces of tile t + 1 stay in registers from the phase that wrote them as rows to the one that writes the image.
template <typename T, int P, int XB, bool KSPLIT>
__global__ __launch_bounds__(128 * P) void attn_wg_dq_kernel(const AttnOperands<T> a, const T* __restrict__ dout,
                                                             const float* __restrict__ lse, const float* __restrict__ delta,
                                                             int64_t items, int nblk, float c2, float scale,
                                                             T* __restrict__ dq_out, int64_t dq_stride, const AttnKSplit ks) {
  typedef typename AFrag<T>::type frag;
  constexpr int D = 128, NS = kPairCols / 16, NMB = kPairCols / 32, NPC = 4 / P;
  __shared__ __attribute__((aligned(16))) T kr[2][kWgRows];
  __shared__ __attribute__((aligned(16))) T vr[2][kWgRows];
  __shared__ __attribute__((aligned(16))) T kt[2][kWgTr];
  __shared__ __attribute__((aligned(16))) float xs[XB][2 * P][2][kPairTile];  // [buffer][wave][S^T, dP^T]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int col0 = kPairCols * (wave & 1);
  const int heads = a.heads;
  const int64_t qp = a.q_stride, kp = a.kv_stride, opitch = (int64_t)heads * D;
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    AttnItem w;
    int split = 0, k_beg = 0;
    if (KSPLIT) {
      const int64_t t = id / heads;
      split = (int)(t % ks.k_splits);
      attn_item((t / ks.k_splits) * heads + id % heads, nblk, heads, a.cu_q, a.cu_k, w, kAttnTile * P);
    } else {
      attn_item(id, nblk, heads, a.cu_q, a.cu_k, w, kAttnTile * P);
    }
    if (w.b0 >= w.len_q) continue;  // (the same for every wave of the workgroup: no barrier is passed by)
    int k_end = w.len_k;
    if (KSPLIT) attn_key_share(w.len_k, ks.k_splits, split, k_beg, k_end);
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D + col0;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D;
    const T* dO = dout + w.beg_q * opitch + (int64_t)w.hd * D + col0;
    const int row = w.b0 + kAttnTile * (wave >> 1) + r;
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
    if (k_beg < k_end) {  // (uniform: one sequence, one share)
      frag kn[NPC], vn[NPC], kh[NPC];
      load_pieces<T, NPC>(kn, k, kp, k_beg, w.len_k, tid);
      load_pieces<T, NPC>(vn, v, kp, k_beg, w.len_k, tid);
      put_row_pieces<T, NPC>(kr[0], kn, tid);
      put_row_pieces<T, NPC>(vr[0], vn, tid);
      put_tr_pieces<T, NPC>(kt[0], kn, tid);
      if (k_beg + kAttnTile < k_end) {
        load_pieces<T, NPC>(kh, k, kp, k_beg + kAttnTile, w.len_k, tid);
        load_pieces<T, NPC>(vn, v, kp, k_beg + kAttnTile, w.len_k, tid);
        put_row_pieces<T, NPC>(kr[1], kh, tid);
        put_row_pieces<T, NPC>(vr[1], vn, tid);
      }
      __syncthreads();  // tiles 0 and 1 are staged
      a_f32x16 st = rows_times<T>(kr[0], qf, r, h, col0), dpt = rows_times<T>(vr[0], df, r, h, col0);
      put_tile(xs[0][wave][0], st, lane);
      put_tile(xs[0][wave][1], dpt, lane);
      for (int k0 = k_beg, cur = 0; k0 < k_end; k0 += kAttnTile, cur ^= 1) {
        const bool more1 = k0 + kAttnTile < k_end, more2 = k0 + 2 * kAttnTile < k_end;
        if (more2) {  // in flight during this tile's MFMAs
          load_pieces<T, NPC>(kn, k, kp, k0 + 2 * kAttnTile, w.len_k, tid);
          load_pieces<T, NPC>(vn, v, kp, k0 + 2 * kAttnTile, w.len_k, tid);
        }
        __syncthreads();  // this tile's partials and image are written
        const int xb = XB == 2 ? cur : 0;
        add_tile(st, xs[xb][wave ^ 1][0], lane);
        add_tile(dpt, xs[xb][wave ^ 1][1], lane);
        // rows are keys, the lane's column its query; keys past len_k get p = 0 (their K, V rows were staged as zeros)
        float ds[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = k0 + acc_row(i, h) < w.len_k ? __builtin_amdgcn_exp2f(st[i] * c2 - L) : 0.f;
          ds[i] = p * (dpt[i] - E);
        }
        const T* img = kt[cur] + kPairTr * (wave & 1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const frag dsf = acc_frag<T>(ds, s);
#pragma unroll
          for (int mb = 0; mb < NMB; ++mb) dq[mb] = AFrag<T>::mfma(read_tr<T>(img, mb, s, r, h), dsf, dq[mb]);
        }
        if (more1) {
          if (XB == 1) __syncthreads();  // the one exchange buffer has been read by every partner
          st = rows_times<T>(kr[cur ^ 1], qf, r, h, col0);
          dpt = rows_times<T>(vr[cur ^ 1], df, r, h, col0);
          const int xn = XB == 2 ? cur ^ 1 : 0;
          put_tile(xs[xn][wave][0], st, lane);
          put_tile(xs[xn][wave][1], dpt, lane);
          put_tr_pieces<T, NPC>(kt[cur ^ 1], kh, tid);
        }
        if (more2) {
          put_row_pieces<T, NPC>(kr[cur], kn, tid);
          put_row_pieces<T, NPC>(vr[cur], vn, tid);
#pragma unroll
          for (int j = 0; j < NPC; ++j) kh[j] = kn[j];
        }
      }
      __syncthreads();  // the last tile's reads are done before the next item stages its first
    }
    if (!ok) continue;  // (stores only: no barrier follows in this item)
    if (KSPLIT)
      store_dcol_f32<kPairCols>(ks.o + (((int64_t)split * ks.total_q + w.beg_q + row) * heads + w.hd) * D + col0, dq, h);
    else
      store_dcol<T, kPairCols>(dq_out + (w.beg_q + row) * dq_stride + (int64_t)w.hd * D + col0, dq, scale, h);
  }
}

// dK, dV of one (sequence, 32 P-key block, head [, query share]): Q and dO rows, the Q^T and dO^T images and the 32 lse and
// delta values staged once per query tile (lse by threads 0..31, delta by threads 32..63 of the workgroup).
template <typename T, int P, int XB, bool SPLIT>
__global__ __launch_bounds__(128 * P) void attn_wg_dkdv_kernel(const AttnOperands<T> a, const T* __restrict__ dout,
                                                               const float* __restrict__ lse, const float* __restrict__ delta,
                                                               int64_t items, int nblk, float c2, float scale,
                                                               T* __restrict__ dk_out, T* __restrict__ dv_out,
                                                               int64_t dkv_stride, int q_splits, int64_t total_k,
                                                               float* __restrict__ part) {
  typedef typename AFrag<T>::type frag;
  constexpr int D = 128, NS = kPairCols / 16, NMB = kPairCols / 32, NPC = 4 / P;
  __shared__ __attribute__((aligned(16))) T qr[2][kWgRows];
  __shared__ __attribute__((aligned(16))) T dr[2][kWgRows];
  __shared__ __attribute__((aligned(16))) T qt[2][kWgTr];
  __shared__ __attribute__((aligned(16))) T dot[2][kWgTr];
  __shared__ __attribute__((aligned(16))) float s_ld[2][2][kAttnTile];        // [buffer][lse, delta]
  __shared__ __attribute__((aligned(16))) float xs[XB][2 * P][2][kPairTile];  // [buffer][wave][S, dP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int col0 = kPairCols * (wave & 1);
  const int heads = a.heads;
  const int64_t qp = a.q_stride, kp = a.kv_stride, opitch = (int64_t)heads * D;
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    AttnItem w;
    int split = 0;
    if (SPLIT) {
      const int64_t t = id / heads;
      split = (int)(t % q_splits);
      attn_item((t / q_splits) * heads + id % heads, nblk, heads, a.cu_q, a.cu_k, w, kAttnTile * P);
    } else {
      attn_item(id, nblk, heads, a.cu_q, a.cu_k, w, kAttnTile * P);
    }
    if (w.b0 >= w.len_k) continue;  // (the same for every wave of the workgroup: no barrier is passed by)
    int q_beg = 0, q_end = w.len_q;
    if (SPLIT) attn_key_share(w.len_q, q_splits, split, q_beg, q_end);
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D + col0;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D + col0;
    const T* dO = dout + w.beg_q * opitch + (int64_t)w.hd * D;
    const int key = w.b0 + kAttnTile * (wave >> 1) + r;  // past the end: zero rows, p = 0, nothing is stored
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
    // thread tid < 64 stages lse (tid < 32) or delta of query row q0 + (tid & 31): the values the pair kernels stage
    const auto row_stat = [&](int q0) -> float {
      const int qr_ = q0 + r;
      const bool in = qr_ < w.len_q;
      const int64_t t = w.beg_q + qr_;
      if (h == 0) {
        const float Lq = in ? lse[t * heads + w.hd] : 0.f;
        return Lq > -INFINITY ? Lq * kLog2e : INFINITY;  // +inf: p = exp2(-inf) = 0
      }
      return in ? delta[t * heads + w.hd] : 0.f;
    };
    if (q_beg < q_end) {  // (uniform: one sequence, one share)
      frag qn[NPC], dn[NPC], qh[NPC], dh[NPC];
      float sn = 0.f;
      load_pieces<T, NPC>(qn, q, qp, q_beg, w.len_q, tid);
      load_pieces<T, NPC>(dn, dO, opitch, q_beg, w.len_q, tid);
      put_row_pieces<T, NPC>(qr[0], qn, tid);
      put_row_pieces<T, NPC>(dr[0], dn, tid);
      put_tr_pieces<T, NPC>(qt[0], qn, tid);
      put_tr_pieces<T, NPC>(dot[0], dn, tid);
      if (wave == 0) s_ld[0][h][r] = row_stat(q_beg);
      if (q_beg + kAttnTile < q_end) {
        load_pieces<T, NPC>(qh, q, qp, q_beg + kAttnTile, w.len_q, tid);
        load_pieces<T, NPC>(dh, dO, opitch, q_beg + kAttnTile, w.len_q, tid);
        put_row_pieces<T, NPC>(qr[1], qh, tid);
        put_row_pieces<T, NPC>(dr[1], dh, tid);
      }
      __syncthreads();  // tiles 0 and 1 are staged
      a_f32x16 sc = rows_times<T>(qr[0], kf, r, h, col0), dp = rows_times<T>(dr[0], vf, r, h, col0);
      put_tile(xs[0][wave][0], sc, lane);
      put_tile(xs[0][wave][1], dp, lane);
      for (int q0 = q_beg, cur = 0; q0 < q_end; q0 += kAttnTile, cur ^= 1) {
        const bool more1 = q0 + kAttnTile < q_end, more2 = q0 + 2 * kAttnTile < q_end;
        if (more2) {  // in flight during this tile's MFMAs
          load_pieces<T, NPC>(qn, q, qp, q0 + 2 * kAttnTile, w.len_q, tid);
          load_pieces<T, NPC>(dn, dO, opitch, q0 + 2 * kAttnTile, w.len_q, tid);
        }
        if (more1 && wave == 0) sn = row_stat(q0 + kAttnTile);
        __syncthreads();  // this tile's partials, images, lse and delta are written
        const int xb = XB == 2 ? cur : 0;
        add_tile(sc, xs[xb][wave ^ 1][0], lane);
        add_tile(dp, xs[xb][wave ^ 1][1], lane);
        // Rows of sc / dp are queries, the lane's column is its key.  Query rows past len_q carry Q = dO = 0, lse =
        // delta = 0: p = 1, dS = 0, and their dO^T / Q^T columns are zero, so they add nothing.  Keys past len_k: p = 0.
        float p[16], ds[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 Lq = *reinterpret_cast<const float4*>(s_ld[cur][0] + 8 * g + 4 * h);
          const float4 Eq = *reinterpret_cast<const float4*>(s_ld[cur][1] + 8 * g + 4 * h);
          const float Lv[4] = {Lq.x, Lq.y, Lq.z, Lq.w}, Ev[4] = {Eq.x, Eq.y, Eq.z, Eq.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int i = 4 * g + e;
            p[i] = key < w.len_k ? __builtin_amdgcn_exp2f(sc[i] * c2 - Lv[e]) : 0.f;
            ds[i] = p[i] * (dp[i] - Ev[e]);
          }
        }
        const T* qimg = qt[cur] + kPairTr * (wave & 1);
        const T* dimg = dot[cur] + kPairTr * (wave & 1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const frag pf = acc_frag<T>(p, s), dsf = acc_frag<T>(ds, s);
#pragma unroll
          for (int mb = 0; mb < NMB; ++mb) {
            dv[mb] = AFrag<T>::mfma(read_tr<T>(dimg, mb, s, r, h), pf, dv[mb]);
            dk[mb] = AFrag<T>::mfma(read_tr<T>(qimg, mb, s, r, h), dsf, dk[mb]);
          }
        }
        if (more1) {
          if (XB == 1) __syncthreads();  // the one exchange buffer has been read by every partner
          sc = rows_times<T>(qr[cur ^ 1], kf, r, h, col0);
          dp = rows_times<T>(dr[cur ^ 1], vf, r, h, col0);
          const int xn = XB == 2 ? cur ^ 1 : 0;
          put_tile(xs[xn][wave][0], sc, lane);
          put_tile(xs[xn][wave][1], dp, lane);
          put_tr_pieces<T, NPC>(qt[cur ^ 1], qh, tid);
          put_tr_pieces<T, NPC>(dot[cur ^ 1], dh, tid);
          if (wave == 0) s_ld[cur ^ 1][h][r] = sn;
        }
        if (more2) {
          put_row_pieces<T, NPC>(qr[cur], qn, tid);
          put_row_pieces<T, NPC>(dr[cur], dn, tid);
#pragma unroll
          for (int j = 0; j < NPC; ++j) qh[j] = qn[j], dh[j] = dn[j];
        }
      }
      __syncthreads();  // the last tile's reads are done before the next item stages its first
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

// ---- host -----------------------------------------------------------------------------------------------------------
// Wave pairs per workgroup and exchange buffers of each kernel as launched (the table in the header comment).
constexpr int kWgFwdP = 4, kWgFwdXB = 2;
constexpr int kWgDqP = 4, kWgDqXB = 1;
constexpr int kWgDkdvP = 2, kWgDkdvXB = 2;
static inline int wg_blocks(int max_seqlen, int pairs) { return (max_seqlen + kAttnTile * pairs - 1) / (kAttnTile * pairs); }

template <typename T>
static int attn_wg_fwd_t(const AttnCall& c, void* out, float* lse, const AttnKSplit& ks, hipStream_t s) {
  constexpr int D = 128;
  const int nblk = wg_blocks(c.max_q, kWgFwdP);
  const int64_t items = c.num_seqs * nblk * c.heads * ks.k_splits;
  const AttnOperands<T> a = attn_operands<T>(c);
  const float c2 = c.scale * kLog2e;
  const dim3 wg(kPairThreads * kWgFwdP);
  if (items > 0) {
    if (ks.k_splits > 1) {
      hipLaunchKernelGGL((attn_wg_fwd_kernel<T, kWgFwdP, kWgFwdXB, true>), dim3(pair_grid(items)), wg, 0, s, a, items, nblk, c2,
                         (T*)out, lse, ks);
      const int64_t n = c.total_q * c.heads * (D / 4);
      hipLaunchKernelGGL((attn_fwd_combine_kernel<T, D>), dim3(pair_grid((n + 255) / 256)), dim3(256), 0, s, ks, c.cu_q,
                         c.num_seqs, c.heads, (T*)out, lse);
    } else {
      hipLaunchKernelGGL((attn_wg_fwd_kernel<T, kWgFwdP, kWgFwdXB, false>), dim3(pair_grid(items)), wg, 0, s, a, items, nblk, c2,
                         (T*)out, lse, ks);
    }
  }
  return hipGetLastError() == hipSuccess ? WCN_SUCCESS : WCN_ERROR_KERNEL_EXECUTION;
}

template <typename T>
static int attn_wg_bwd_t(const AttnCall& c, const void* dout, const void* out, const float* lse, void* dq, int64_t dq_stride,
                         void* dk, void* dv, int64_t dkv_stride, int q_splits, float* part, float* delta, const AttnKSplit& ks,
                         hipStream_t s) {
  constexpr int D = 128;
  const AttnOperands<T> a = attn_operands<T>(c);
  const float c2 = c.scale * kLog2e;
  const int64_t rows = c.total_q * c.heads;
  const int nblk_q = wg_blocks(c.max_q, kWgDqP), nblk_k = wg_blocks(c.max_k, kWgDkdvP);
  const int64_t items_q = c.num_seqs * nblk_q * c.heads, items_k = c.num_seqs * nblk_k * c.heads;
  const dim3 wg_q(kPairThreads * kWgDqP), wg_k(kPairThreads * kWgDkdvP);
  if (rows > 0)
    hipLaunchKernelGGL((attn_delta_kernel<T, D>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, (const T*)dout,
                       (const T*)out, rows, delta);
  if (items_k > 0 && c.total_k > 0) {
    if (q_splits > 1) {
      hipLaunchKernelGGL((attn_wg_dkdv_kernel<T, kWgDkdvP, kWgDkdvXB, true>), dim3(pair_grid(items_k * q_splits)), wg_k, 0, s, a,
                         (const T*)dout, lse, (const float*)delta, items_k * q_splits, nblk_k, c2, c.scale, (T*)dk, (T*)dv,
                         dkv_stride, q_splits, c.total_k, part);
      const int64_t n = c.total_k * 2 * c.heads * (D / 4);
      hipLaunchKernelGGL((attn_dkdv_reduce_kernel<T, D>), dim3(pair_grid((n + 255) / 256)), dim3(256), 0, s, (const float*)part,
                         c.cu_k, c.num_seqs, c.total_k, c.heads, q_splits, c.scale, (T*)dk, (T*)dv, dkv_stride);
    } else {
      hipLaunchKernelGGL((attn_wg_dkdv_kernel<T, kWgDkdvP, kWgDkdvXB, false>), dim3(pair_grid(items_k)), wg_k, 0, s, a,
                         (const T*)dout, lse, (const float*)delta, items_k, nblk_k, c2, c.scale, (T*)dk, (T*)dv, dkv_stride, 1,
                         c.total_k, (float*)nullptr);
    }
  }
  if (items_q > 0 && c.total_q > 0) {
    if (ks.k_splits > 1) {
      const int64_t items = items_q * ks.k_splits;
      hipLaunchKernelGGL((attn_wg_dq_kernel<T, kWgDqP, kWgDqXB, true>), dim3(pair_grid(items)), wg_q, 0, s, a, (const T*)dout, lse,
                         (const float*)delta, items, nblk_q, c2, c.scale, (T*)dq, dq_stride, ks);
      const int64_t n = c.total_q * c.heads * (D / 4);
      hipLaunchKernelGGL((attn_dq_reduce_kernel<T, D>), dim3(pair_grid((n + 255) / 256)), dim3(256), 0, s, ks, c.cu_q, c.num_seqs,
                         c.heads, c.scale, (T*)dq, dq_stride);
    } else {
      hipLaunchKernelGGL((attn_wg_dq_kernel<T, kWgDqP, kWgDqXB, false>), dim3(pair_grid(items_q)), wg_q, 0, s, a, (const T*)dout,
                         lse, (const float*)delta, items_q, nblk_q, c2, c.scale, (T*)dq, dq_stride, ks);
    }
  }
  return hipGetLastError() == hipSuccess ? WCN_SUCCESS : WCN_ERROR_KERNEL_EXECUTION;
}

int attn_wg_fwd(int dtype, const AttnCall& c, void* out, float* lse, const AttnKSplit& ks, hipStream_t s) {
  return with_dtype16(dtype, [&](auto t) { return attn_wg_fwd_t<decltype(t)>(c, out, lse, ks, s); });
}

int attn_wg_bwd(int dtype, const AttnCall& c, const void* dout, const void* out, const float* lse, void* dq, int64_t dq_stride,
                void* dk, void* dv, int64_t dkv_stride, int q_splits, float* part, float* delta, const AttnKSplit& ks,
                hipStream_t s) {
  return with_dtype16(dtype, [&](auto t) {
    return attn_wg_bwd_t<decltype(t)>(c, dout, out, lse, dq, dq_stride, dk, dv, dkv_stride, q_splits, part, delta, ks, s);
  });
}
}  // namespace wcn
