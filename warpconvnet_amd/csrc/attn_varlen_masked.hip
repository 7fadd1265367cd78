// attn_varlen_masked.hip - the separate-operand varlen attention of attn_varlen.hip with a per-(query, key) block mask that
// all heads share: the masked cross-attention of a Mask2Former-style query decoder (each query attends only to the points its
// previous mask prediction marked foreground), and the kernel that packs the mask.  Kernels of their own on the helpers of
// attn_varlen.h: attn_varlen.hip is not touched, so an unmasked call keeps its code, its registers and its bits.
//
// The mask.  One bit per (query, key) pair of a sequence, 1 = blocked, stored twice so that every kernel reads one 32-bit word
// per lane and score tile:
//   q_words [Tq, q_pitch]  bit j of word w of query row t = key 32 w + j of t's sequence   (forward, dQ: query on the lane)
//   k_words [Tk, k_pitch]  bit j of word w of key row t   = query 32 w + j of t's sequence (dK/dV: key on the lane)
// Bits past the end of a sequence's keys / queries are 0 in both; the kernels exclude those positions by length.
// attn_mask_pack_kernel: a workgroup of 256 threads owns one (sequence, 32-key tile, 32-query tile) of the source - logits
// [Tk, Q] (blocked <=> logit < threshold) or a uint8 bool tensor of that shape, rows optionally picked through key_index.
// Half a wave reads 32 consecutive columns of one key row (coalesced along Q), a ballot turns two key rows into two words of
// the key layout, the 32 words go to LDS, and thread t < 32 writes word t of each layout: its key's word as it stands and its
// query's word as the transposed column.  Every word of every in-sequence row is written exactly once; no atomics.
// attn_mask_release_kernel (second launch, release_full_rows): a workgroup owns (sequence, 32-query tile); eight threads scan a
// query's words, a query whose every in-range key is blocked is "released": its q_words are cleared and its bit is cleared in
// word `tile` of every key row of the sequence - a column of k_words only this workgroup writes.  Integer work, fixed order.
//
// Forward and dQ (attn_fwd_masked_kernel, attn_bwd_dq_masked_kernel): the four-wave staged-tile structure of the shared
// kernels - 128 query rows per workgroup, wave w on rows 32 w .. 32 w + 31, every 32-key tile of K (row-major) and V^T / K^T
// (transposed) staged once in LDS, double-buffered, one barrier per tile - on the split-key work item (sequence, query block,
// split, head).  A lane loads the one word of its query for the NEXT key tile while the current one is multiplied; keys past
// the sequence end are OR-ed into it as blocked, a query row past the end has every bit set.  After the S^T chain a blocked
// score becomes -inf before the running maximum.  A query that has not seen an allowed key yet has m = -inf and a tile maximum
// of -inf: the tile then runs with alpha = 1, p = exp2(-inf - 0) = 0 and l unchanged (never exp2(-inf - (-inf))).
// Tile skip: a wave whose 32 lanes all hold a full word skips the tile's MFMAs, exps and rescale - exactly what the arithmetic
// would have done (alpha = 1, ls = 0, m and the accumulator unchanged), so no bit depends on the skip.  It still stages and
// reaches the barrier.  The staging loads themselves are never skipped (that would need the four waves' words a tile early in
// LDS; not measured, not built).
// dK/dV (attn_bwd_dkdv_masked_kernel): one wave per (sequence, 32-key block, head) sweeps the query blocks and reads k_words;
// P is recomputed from the final LSE with blocked pairs at exactly 0; a query block the wave's 32 keys are all blocked from
// is skipped before its loads.  No q_splits: the query side is a few blocks long.
// A query with no allowed key (release off, or len_k = 0): out = 0, lse = -inf, dq = 0, nothing added to dk / dv - the empty
// side of attn_varlen.hip; the backward maps lse = -inf to +inf in the exp2 domain so p = exp2(-inf) = 0.  A key every query
// blocks gets dk = dv = 0.  Deterministic: no float atomics, fixed orders, a sequence's result does not depend on its batch.
// With no bit set each wave issues the unmasked kernels' arithmetic on its rows: the same bits as attn_varlen.hip.
#include "attn_varlen.h"

namespace wcn {

constexpr int kMaskTile = kAttnTile;              // keys / queries of one mask word
constexpr int kMaskWaves = 4;
constexpr int kMaskWgRows = kMaskWaves * kMaskTile;  // query rows of a forward / dQ work item
constexpr int64_t kMaskMaxGrid = 1 << 22;

struct AttnMaskWords {
  const uint32_t *qw, *kw;
  int64_t qp, kp;  // row pitches, words
};

// ---- packing --------------------------------------------------------------------------------------------------------------
template <typename S>
__device__ __forceinline__ bool mask_blocked(S x, float thr) { return (float)x < thr; }
template <>
__device__ __forceinline__ bool mask_blocked<uint8_t>(uint8_t x, float) { return x != 0; }

template <typename S>
__global__ __launch_bounds__(256) void attn_mask_pack_kernel(const S* __restrict__ src, int64_t src_rows, int64_t src_pitch,
                                                             int q_cols, float thr, const int32_t* __restrict__ key_index,
                                                             const int32_t* __restrict__ cu_q, const int32_t* __restrict__ cu_k,
                                                             int64_t items, int nq, int nk, uint32_t* __restrict__ q_words,
                                                             int64_t q_pitch, uint32_t* __restrict__ k_words, int64_t k_pitch) {
  __shared__ uint32_t s_bits[kMaskTile];  // word of key row i of the tile: bit j = query j of the tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, sub = lane >> 5;
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    const int qt = (int)(id % nq);
    const int64_t t = id / nq;
    const int kt = (int)(t % nk);
    const int64_t seq = t / nk;
    const int64_t beg_q = cu_q[seq], beg_k = cu_k[seq];
    const int len_q = cu_q[seq + 1] - (int)beg_q, len_k = cu_k[seq + 1] - (int)beg_k;
    const int q0 = kMaskTile * qt, k0 = kMaskTile * kt;
    if (q0 >= len_q && k0 >= len_k) continue;  // no row of either layout has this word
    const int qc = q0 + col;
    const bool q_ok = qc < len_q && qc < q_cols;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kr = 8 * wave + 2 * i + sub;
      bool b = false;
      if (q_ok && k0 + kr < len_k) {
        int64_t row = beg_k + k0 + kr;
        if (key_index) row = key_index[row];
        row = row < 0 ? 0 : (row < src_rows ? row : src_rows - 1);  // a bad index reads a wrong row, never outside the source
        b = mask_blocked<S>(src[row * src_pitch + qc], thr);
      }
      const uint64_t bal = __ballot(b);
      if (lane == 0) {
        s_bits[8 * wave + 2 * i] = (uint32_t)bal;
        s_bits[8 * wave + 2 * i + 1] = (uint32_t)(bal >> 32);
      }
    }
    __syncthreads();
    if (tid < kMaskTile) {
      if (k0 + tid < len_k) k_words[(beg_k + k0 + tid) * k_pitch + qt] = s_bits[tid];
      if (q0 + tid < len_q) {
        uint32_t w = 0;
#pragma unroll
        for (int k = 0; k < kMaskTile; ++k) w |= ((s_bits[k] >> tid) & 1u) << k;
        q_words[(beg_q + q0 + tid) * q_pitch + kt] = w;
      }
    }
    __syncthreads();  // s_bits is written again by the next item
  }
}

__global__ __launch_bounds__(256) void attn_mask_release_kernel(const int32_t* __restrict__ cu_q, const int32_t* __restrict__ cu_k,
                                                                int64_t items, int nq, uint32_t* __restrict__ q_words,
                                                                int64_t q_pitch, uint32_t* __restrict__ k_words,
                                                                int64_t k_pitch) {
  __shared__ uint32_t s_rel[kMaskWaves];  // wave w: bit j = query 8 w + j of the tile is released
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qi = tid >> 3, part = tid & 7;  // eight threads scan the words of query qi of the tile
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    const int qt = (int)(id % nq);
    const int64_t seq = id / nq;
    const int64_t beg_q = cu_q[seq], beg_k = cu_k[seq];
    const int len_q = cu_q[seq + 1] - (int)beg_q, len_k = cu_k[seq + 1] - (int)beg_k;
    const int q0 = kMaskTile * qt;
    if (q0 >= len_q || len_k == 0) continue;  // no key: nothing is set
    const int nw = (len_k + kMaskTile - 1) / kMaskTile;
    bool full = q0 + qi < len_q;
    if (full) {
      const uint32_t* rowp = q_words + (beg_q + q0 + qi) * q_pitch;
      for (int w = part; w < nw; w += 8) {
        const uint32_t need = (w == nw - 1 && (len_k & 31)) ? (1u << (len_k & 31)) - 1u : ~0u;
        if ((rowp[w] & need) != need) full = false;
      }
    }
    const uint64_t bal = __ballot(full);
    if (lane == 0) {
      uint32_t rel = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (((bal >> (8 * j)) & 0xffu) == 0xffu) rel |= 1u << j;
      s_rel[wave] = rel;
    }
    __syncthreads();  // every scan of this tile's rows is done before any of them is cleared
    const uint32_t rel = s_rel[0] | (s_rel[1] << 8) | (s_rel[2] << 16) | (s_rel[3] << 24);
    if (rel) {
      for (int i = tid; i < kMaskTile * nw; i += 256) {
        const int j = i / nw, w = i % nw;
        if ((rel >> j) & 1u) q_words[(beg_q + q0 + j) * q_pitch + w] = 0u;
      }
      for (int k = tid; k < len_k; k += 256) {
        uint32_t* p = k_words + (beg_k + k) * k_pitch + qt;  // word qt of a key row: written by this workgroup alone
        *p &= ~rel;
      }
    }
    __syncthreads();  // s_rel is written again by the next item
  }
}

// ---- staged tiles (the layout of the shared kernels of attn_varlen.hip) ------------------------------------------------------
template <int D>
struct MaskedTile {
  static constexpr int kRowPitch = D + 8;                        // row-major image: 16-B aligned rows, elements
  static constexpr int kRows = kMaskTile * kRowPitch;            // elements of a row-major image
  static constexpr int kTr = ((D + 31) / 32) * 32 * kAttnPitch;  // elements of a transposed image
};
template <typename T, int D>
__device__ __forceinline__ void tile_put_rows(T* __restrict__ rows, const typename AFrag<T>::type& v, int row, int dch) {
  *reinterpret_cast<typename AFrag<T>::type*>(rows + row * MaskedTile<D>::kRowPitch + 8 * dch) = v;
}
template <typename T>
__device__ __forceinline__ void tile_put_tr(T* __restrict__ img, const typename AFrag<T>::type& v, int row, int dch) {
#pragma unroll
  for (int e = 0; e < 8; ++e) img[(8 * dch + e) * kAttnPitch + row] = v[e];
}
template <typename T, int D>
__device__ __forceinline__ typename AFrag<T>::type tile_get_row(const T* __restrict__ rows, int r, int s, int h) {
  return *reinterpret_cast<const typename AFrag<T>::type*>(rows + r * MaskedTile<D>::kRowPitch + 16 * s + 8 * h);
}

// The blocked word of a query row for the key tile at k0: the mask word, keys past len_k set; a row past len_q: all set.
__device__ __forceinline__ uint32_t query_word(const uint32_t* __restrict__ mrow, bool ok, int k0, int len_k) {
  if (!ok) return ~0u;
  uint32_t x = mrow[k0 >> 5];
  const int left = len_k - k0;
  if (left < kMaskTile) x |= ~0u << left;  // 1 <= left here: k0 is inside the sweep
  return x;
}

// The work item of a flat id of the forward / dQ sweep: (sequence, 128-query block, [split,] head) and the keys it sweeps.
template <bool KSPLIT>
__device__ __forceinline__ void masked_item(int64_t id, int nblk, const int32_t* cu_q, const int32_t* cu_k, int heads,
                                            const AttnKSplit& ks, AttnItem& w, int& split, int& k_beg, int& k_end) {
  split = 0;
  if (KSPLIT) {
    const int64_t t = id / heads;
    split = (int)(t % ks.k_splits);
    attn_item((t / ks.k_splits) * heads + id % heads, nblk, heads, cu_q, cu_k, w, kMaskWgRows);
  } else {
    attn_item(id, nblk, heads, cu_q, cu_k, w, kMaskWgRows);
  }
  k_beg = 0, k_end = w.len_k;
  if (KSPLIT) attn_key_share(w.len_k, ks.k_splits, split, k_beg, k_end);
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
template <typename T, int D, bool KSPLIT>
__global__ __launch_bounds__(256) void attn_fwd_masked_kernel(const AttnOperands<T> a, const AttnMaskWords mk, int64_t items,
                                                              int nblk, float c2, T* __restrict__ out, float* __restrict__ lse,
                                                              const AttnKSplit ks) {
  typedef typename AFrag<T>::type frag;
  typedef MaskedTile<D> Tile;
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
    int split, k_beg, k_end;
    masked_item<KSPLIT>(id, nblk, a.cu_q, a.cu_k, heads, ks, w, split, k_beg, k_end);
    if (w.b0 >= w.len_q) continue;  // (the same for every wave of the workgroup)
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D;
    const int row = w.b0 + kMaskTile * wave + r;  // past the end: zeros, every key blocked, nothing stored
    const bool ok = row < w.len_q;
    const uint32_t* mrow = mk.qw + (w.beg_q + row) * mk.qp;
    frag qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = load8<T>(q, qp, row, w.len_q, 16 * s + 8 * h);
    a_f32x16 acc[NMB];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mb][i] = 0.f;
    float m = -INFINITY, l = 0.f;
    frag kreg, vreg;
    uint32_t wnext = ~0u;
    if (k_beg < k_end) {
      wnext = query_word(mrow, ok, k_beg, w.len_k);
      if (stager) {
        tile_put_rows<T, D>(kr[0], load8<T>(k, kp, k_beg + srow, w.len_k, 8 * sdch), srow, sdch);
        tile_put_tr<T>(vt[0], load8<T>(v, kp, k_beg + srow, w.len_k, 8 * sdch), srow, sdch);
      }
    }
    __syncthreads();
    for (int k0 = k_beg, cur = 0; k0 < k_end; k0 += kMaskTile, cur ^= 1) {
      const bool last = k0 + kMaskTile >= k_end;
      const bool more = stager && !last;
      const uint32_t blk = wnext;
      if (more) {  // the next tile's loads are in flight during this tile's MFMAs
        kreg = load8<T>(k, kp, k0 + kMaskTile + srow, w.len_k, 8 * sdch);
        vreg = load8<T>(v, kp, k0 + kMaskTile + srow, w.len_k, 8 * sdch);
      }
      if (!last) wnext = query_word(mrow, ok, k0 + kMaskTile, w.len_k);
      if (!__all(blk == ~0u)) {  // (wave-uniform) some query of this wave sees some key of the tile
        a_f32x16 st;
#pragma unroll
        for (int i = 0; i < 16; ++i) st[i] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) st = AFrag<T>::mfma(tile_get_row<T, D>(kr[cur], r, s, h), qf[s], st);
        float x[16];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          x[i] = (blk >> acc_row(i, h)) & 1u ? -INFINITY : st[i] * c2;
          mx = fmaxf(mx, x[i]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(m, mx);
        const bool live = mn > -INFINITY;  // false: no allowed key so far - alpha = 1, p = 0, l and m as they are
        const float base = live ? mn : 0.f;
        const float alpha = live ? __builtin_amdgcn_exp2f(m - mn) : 1.f;
        float ls = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          x[i] = __builtin_amdgcn_exp2f(x[i] - base);
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
      }
      if (more) {
        tile_put_rows<T, D>(kr[cur ^ 1], kreg, srow, sdch);
        tile_put_tr<T>(vt[cur ^ 1], vreg, srow, sdch);
      }
      __syncthreads();  // the next tile is staged, and this tile's reads are done before its buffer is written again
    }
    if (KSPLIT) {
      // the share's state as it stands: a share without an allowed key leaves m = -inf, l = 0 and a zero accumulator
      if (ok) {
        const int64_t idx = ((int64_t)split * ks.total_q + w.beg_q + row) * heads + w.hd;
        store_dcol_f32<D>(ks.o + idx * D, acc, h);
        if (h == 0) *reinterpret_cast<float2*>(ks.ml + 2 * idx) = make_float2(m, l);
      }
    } else if (ok) {
      // l > 0 once the query has seen an allowed key (its row maximum contributes exp2(0) = 1); none: the accumulator is
      // still zero and is stored as exact zeros, lse = -inf
      const bool any = m > -INFINITY;
      const int64_t t = w.beg_q + row;
      store_dcol<T, D>(out + (t * heads + w.hd) * D, acc, any ? 1.f / l : 0.f, h);
      if (h == 0) lse[t * heads + w.hd] = any ? (m + __log2f(l)) * kLn2 : -INFINITY;
    }
  }
}

// ---- dQ -----------------------------------------------------------------------------------------------------------------------
template <typename T, int D, bool KSPLIT>
__global__ __launch_bounds__(256) void attn_bwd_dq_masked_kernel(const AttnOperands<T> a, const AttnMaskWords mk,
                                                                 const T* __restrict__ dout, const float* __restrict__ lse,
                                                                 const float* __restrict__ delta, int64_t items, int nblk,
                                                                 float c2, float scale, T* __restrict__ dq_out,
                                                                 int64_t dq_stride, const AttnKSplit ks) {
  typedef typename AFrag<T>::type frag;
  typedef MaskedTile<D> Tile;
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
    int split, k_beg, k_end;
    masked_item<KSPLIT>(id, nblk, a.cu_q, a.cu_k, heads, ks, w, split, k_beg, k_end);
    if (w.b0 >= w.len_q) continue;
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D;
    const T* dO = dout + w.beg_q * opitch + (int64_t)w.hd * D;
    const int row = w.b0 + kMaskTile * wave + r;
    const bool ok = row < w.len_q;
    const uint32_t* mrow = mk.qw + (w.beg_q + row) * mk.qp;
    frag qf[NS], df[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      qf[s] = load8<T>(q, qp, row, w.len_q, 16 * s + 8 * h);
      df[s] = load8<T>(dO, opitch, row, w.len_q, 16 * s + 8 * h);
    }
    // lse = -inf marks a query with no allowed key: +inf here makes its p = exp2(-inf) = 0, so its dq stays zero and a
    // -inf never meets the subtraction below
    float L = ok ? lse[(w.beg_q + row) * heads + w.hd] : 0.f;
    L = L > -INFINITY ? L * kLog2e : INFINITY;
    const float E = ok ? delta[(w.beg_q + row) * heads + w.hd] : 0.f;
    a_f32x16 dq[NMB];
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
      for (int i = 0; i < 16; ++i) dq[mb][i] = 0.f;
    frag kreg, vreg;
    uint32_t wnext = ~0u;
    if (k_beg < k_end) {
      wnext = query_word(mrow, ok, k_beg, w.len_k);
      if (stager) {
        kreg = load8<T>(k, kp, k_beg + srow, w.len_k, 8 * sdch);
        tile_put_rows<T, D>(kr[0], kreg, srow, sdch);
        tile_put_tr<T>(kt[0], kreg, srow, sdch);
        tile_put_rows<T, D>(vr[0], load8<T>(v, kp, k_beg + srow, w.len_k, 8 * sdch), srow, sdch);
      }
    }
    __syncthreads();
    for (int k0 = k_beg, cur = 0; k0 < k_end; k0 += kMaskTile, cur ^= 1) {
      const bool last = k0 + kMaskTile >= k_end;
      const bool more = stager && !last;
      const uint32_t blk = wnext;
      if (more) {
        kreg = load8<T>(k, kp, k0 + kMaskTile + srow, w.len_k, 8 * sdch);
        vreg = load8<T>(v, kp, k0 + kMaskTile + srow, w.len_k, 8 * sdch);
      }
      if (!last) wnext = query_word(mrow, ok, k0 + kMaskTile, w.len_k);
      if (!__all(blk == ~0u)) {  // otherwise every dS of this wave's tile is zero: nothing to add
        a_f32x16 st, dpt;
#pragma unroll
        for (int i = 0; i < 16; ++i) st[i] = dpt[i] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          st = AFrag<T>::mfma(tile_get_row<T, D>(kr[cur], r, s, h), qf[s], st);
          dpt = AFrag<T>::mfma(tile_get_row<T, D>(vr[cur], r, s, h), df[s], dpt);
        }
        float ds[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = (blk >> acc_row(i, h)) & 1u ? 0.f : __builtin_amdgcn_exp2f(st[i] * c2 - L);
          ds[i] = p * (dpt[i] - E);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const frag dsf = acc_frag<T>(ds, s);
#pragma unroll
          for (int mb = 0; mb < NMB; ++mb) dq[mb] = AFrag<T>::mfma(read_tr<T>(kt[cur], mb, s, r, h), dsf, dq[mb]);
        }
      }
      if (more) {
        tile_put_rows<T, D>(kr[cur ^ 1], kreg, srow, sdch);
        tile_put_tr<T>(kt[cur ^ 1], kreg, srow, sdch);
        tile_put_rows<T, D>(vr[cur ^ 1], vreg, srow, sdch);
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

// ---- dK, dV -------------------------------------------------------------------------------------------------------------------
// Left to itself the compiler takes 202 VGPRs + 64 AGPRs at D = 64 (one wave per SIMD); the two-waves-per-SIMD register target
// gives 211 VGPRs, no AGPRs and no scratch, and measured 15 % off the forward + backward call (docs/OPTIMISATION_LOG.md AW).
template <typename T, int D>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void attn_bwd_dkdv_masked_kernel(const AttnOperands<T> a, const AttnMaskWords mk,
                                                                  const T* __restrict__ dout, const float* __restrict__ lse,
                                                                  const float* __restrict__ delta, int64_t items, int nblk,
                                                                  float c2, float scale, T* __restrict__ dk_out,
                                                                  T* __restrict__ dv_out, int64_t dkv_stride) {
  typedef typename AFrag<T>::type frag;
  constexpr int NS = D / 16, NMB = (D + 31) / 32;
  __shared__ __attribute__((aligned(16))) T qt[NMB * 32 * kAttnPitch];
  __shared__ __attribute__((aligned(16))) T dot[NMB * 32 * kAttnPitch];
  __shared__ __attribute__((aligned(16))) float s_lse[kMaskTile];
  __shared__ __attribute__((aligned(16))) float s_del[kMaskTile];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int heads = a.heads;
  const int64_t qp = a.q_stride, kp = a.kv_stride, opitch = (int64_t)heads * D;
  for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
    AttnItem w;
    attn_item(id, nblk, heads, a.cu_q, a.cu_k, w);
    if (w.b0 >= w.len_k) continue;
    const T* q = a.q + w.beg_q * qp + (int64_t)w.hd * D;
    const T* k = a.k + w.beg_k * kp + (int64_t)w.hd * D;
    const T* v = a.v + w.beg_k * kp + (int64_t)w.hd * D;
    const T* dO = dout + w.beg_q * opitch + (int64_t)w.hd * D;
    const int key = w.b0 + r;
    const bool kin = key < w.len_k;
    const uint32_t* mrow = mk.kw + (w.beg_k + key) * mk.kp;
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
    for (int q0 = 0; q0 < w.len_q; q0 += kMaskTile) {
      // bit j: query q0 + j may not see this lane's key; queries past len_q and a key past len_k count as blocked
      uint32_t blk = kin ? mrow[q0 >> 5] : ~0u;
      if (w.len_q - q0 < kMaskTile) blk |= ~0u << (w.len_q - q0);
      if (__all(blk == ~0u)) continue;  // (uniform over the wave, which is the workgroup) P of the whole tile is zero
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
        // lse = -inf (a query with no allowed key) becomes +inf in the exp2 domain: p = exp2(-inf) = 0
        const int qr = q0 + r;
        const bool ok = qr < w.len_q;
        const int64_t t = w.beg_q + qr;
        if (h == 0) {
          const float L = ok ? lse[t * heads + w.hd] : 0.f;
          s_lse[r] = L > -INFINITY ? L * kLog2e : INFINITY;
        } else {
          s_del[r] = ok ? delta[t * heads + w.hd] : 0.f;
        }
      }
      __syncthreads();
      // rows of sc / dp are queries, the lane's column is its key
      float p[16], ds[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 L = *reinterpret_cast<const float4*>(s_lse + 8 * g + 4 * h);
        const float4 E = *reinterpret_cast<const float4*>(s_del + 8 * g + 4 * h);
        const float Lv[4] = {L.x, L.y, L.z, L.w}, Ev[4] = {E.x, E.y, E.z, E.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g + e;
          p[i] = (blk >> acc_row(i, h)) & 1u ? 0.f : __builtin_amdgcn_exp2f(sc[i] * c2 - Lv[e]);
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
    if (kin) {
      const int64_t off = (w.beg_k + key) * dkv_stride + (int64_t)w.hd * D;
      store_dcol<T, D>(dk_out + off, dk, scale, h);
      store_dcol<T, D>(dv_out + off, dv, 1.f, h);
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
static inline unsigned masked_grid(int64_t items) { return (unsigned)(items < kMaskMaxGrid ? items : kMaskMaxGrid); }
static inline int masked_words(int max_seqlen) { return (max_seqlen + kMaskTile - 1) / kMaskTile; }
static inline int masked_wg_blocks(int max_seqlen) { return (max_seqlen + kMaskWgRows - 1) / kMaskWgRows; }

template <typename T, int D>
static int masked_fwd_t(const AttnCall& c, const AttnMaskWords& mk, void* out, float* lse, const AttnKSplit& ks, hipStream_t s) {
  const int nblk = masked_wg_blocks(c.max_q);
  const int64_t items = c.num_seqs * nblk * c.heads * ks.k_splits;
  const AttnOperands<T> a = attn_operands<T>(c);
  const float c2 = c.scale * kLog2e;
  if (items > 0) {
    if (ks.k_splits > 1) {
      hipLaunchKernelGGL((attn_fwd_masked_kernel<T, D, true>), dim3(masked_grid(items)), dim3(64 * kMaskWaves), 0, s, a, mk, items,
                         nblk, c2, (T*)out, lse, ks);
      const int64_t n = c.total_q * c.heads * (D / 4);
      hipLaunchKernelGGL((attn_fwd_combine_kernel<T, D>), dim3(masked_grid((n + 255) / 256)), dim3(256), 0, s, ks, c.cu_q,
                         c.num_seqs, c.heads, (T*)out, lse);
    } else {
      hipLaunchKernelGGL((attn_fwd_masked_kernel<T, D, false>), dim3(masked_grid(items)), dim3(64 * kMaskWaves), 0, s, a, mk,
                         items, nblk, c2, (T*)out, lse, ks);
    }
  }
  return hipGetLastError() == hipSuccess ? WCN_SUCCESS : WCN_ERROR_KERNEL_EXECUTION;
}

template <typename T, int D>
static int masked_bwd_t(const AttnCall& c, const AttnMaskWords& mk, const void* dout, const void* out, const float* lse, void* dq,
                        int64_t dq_stride, void* dk, void* dv, int64_t dkv_stride, float* delta, const AttnKSplit& ks,
                        hipStream_t s) {
  const AttnOperands<T> a = attn_operands<T>(c);
  const float c2 = c.scale * kLog2e;
  const int64_t rows = c.total_q * c.heads;
  const int nblk_q = masked_wg_blocks(c.max_q), nblk_k = masked_words(c.max_k);
  const int64_t items_q = c.num_seqs * nblk_q * c.heads * ks.k_splits, items_k = c.num_seqs * nblk_k * c.heads;
  if (rows > 0)
    hipLaunchKernelGGL((attn_delta_kernel<T, D>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, (const T*)dout,
                       (const T*)out, rows, delta);
  if (items_k > 0 && c.total_k > 0)
    hipLaunchKernelGGL((attn_bwd_dkdv_masked_kernel<T, D>), dim3(masked_grid(items_k)), dim3(64), 0, s, a, mk, (const T*)dout, lse,
                       (const float*)delta, items_k, nblk_k, c2, c.scale, (T*)dk, (T*)dv, dkv_stride);
  if (items_q > 0 && c.total_q > 0) {
    if (ks.k_splits > 1) {
      hipLaunchKernelGGL((attn_bwd_dq_masked_kernel<T, D, true>), dim3(masked_grid(items_q)), dim3(64 * kMaskWaves), 0, s, a, mk,
                         (const T*)dout, lse, (const float*)delta, items_q, nblk_q, c2, c.scale, (T*)dq, dq_stride, ks);
      const int64_t n = c.total_q * c.heads * (D / 4);
      hipLaunchKernelGGL((attn_dq_reduce_kernel<T, D>), dim3(masked_grid((n + 255) / 256)), dim3(256), 0, s, ks, c.cu_q,
                         c.num_seqs, c.heads, c.scale, (T*)dq, dq_stride);
    } else {
      hipLaunchKernelGGL((attn_bwd_dq_masked_kernel<T, D, false>), dim3(masked_grid(items_q)), dim3(64 * kMaskWaves), 0, s, a, mk,
                         (const T*)dout, lse, (const float*)delta, items_q, nblk_q, c2, c.scale, (T*)dq, dq_stride, ks);
    }
  }
  return hipGetLastError() == hipSuccess ? WCN_SUCCESS : WCN_ERROR_KERNEL_EXECUTION;
}

template <typename F>
static int masked_dispatch(int head_dim, int dtype, F&& f) {
  return with_dtype16(dtype, [&](auto t) {
    switch (head_dim) {
      case 16: return f(t, std::integral_constant<int, 16>{});
      case 32: return f(t, std::integral_constant<int, 32>{});
      default: return f(t, std::integral_constant<int, 64>{});
    }
  });
}

// The mask of a call against its sizes: both layouts present, 4-byte aligned, pitches that hold every word.
static bool masked_words_ok(const void* q_words, int64_t q_pitch, const void* k_words, int64_t k_pitch, int64_t total_q,
                            int64_t total_k, int max_q, int max_k) {
  if (q_pitch < masked_words(max_k) || k_pitch < masked_words(max_q)) return false;
  if ((total_q > 0 && max_k > 0 && !q_words) || (total_k > 0 && max_q > 0 && !k_words)) return false;
  return aligned_to(q_words, 4) && aligned_to(k_words, 4);
}

template <typename S>
static void mask_pack_launch(const void* src, int64_t src_rows, int64_t src_pitch, int q_cols, float thr, const int32_t* key_index,
                             const int32_t* cu_q, const int32_t* cu_k, int64_t items, int nq, int nk, uint32_t* q_words,
                             int64_t q_pitch, uint32_t* k_words, int64_t k_pitch, hipStream_t s) {
  hipLaunchKernelGGL((attn_mask_pack_kernel<S>), dim3(masked_grid(items)), dim3(256), 0, s, (const S*)src, src_rows, src_pitch,
                     q_cols, thr, key_index, cu_q, cu_k, items, nq, nk, q_words, q_pitch, k_words, k_pitch);
}

}  // namespace wcn

using namespace wcn;

int32_t wcn_attn_mask_words(int32_t max_seqlen) { return max_seqlen > 0 ? masked_words(max_seqlen) : 0; }

int wcn_attn_mask_pack(const void* src, int32_t src_dtype, int64_t src_rows, int64_t src_pitch, int32_t q_cols, float threshold,
                       const int32_t* key_index, const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs, int64_t total_q,
                       int64_t total_k, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t release_full_rows, int32_t* q_words,
                       int64_t q_pitch, int32_t* k_words, int64_t k_pitch, wcn_stream_t stream) {
  if (num_seqs < 0 || total_q < 0 || total_k < 0 || src_rows < 0 || q_cols < 0 || max_seqlen_q < 0 || max_seqlen_k < 0 ||
      !(threshold == threshold))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (src_dtype != WCN_F32 && src_dtype != WCN_F16 && src_dtype != WCN_BF16 && src_dtype != WCN_ATTN_MASK_U8)
    return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (total_q > INT32_MAX || total_k > INT32_MAX || src_rows > INT32_MAX) return WCN_ERROR_INVALID_PARAMETERS;
  if (num_seqs > 0 && (!cu_q || !cu_k)) return WCN_ERROR_INVALID_PARAMETERS;
  if (src_pitch < q_cols || max_seqlen_q > q_cols) return WCN_ERROR_INVALID_PARAMETERS;  // column j is query j of a sequence
  if (!key_index && src_rows != total_k) return WCN_ERROR_INVALID_PARAMETERS;         // keys as they lie
  if (total_k > 0 && (!src || src_rows == 0)) return WCN_ERROR_INVALID_PARAMETERS;
  if (!masked_words_ok(q_words, q_pitch, k_words, k_pitch, total_q, total_k, max_seqlen_q, max_seqlen_k))
    return WCN_ERROR_INVALID_PARAMETERS;
  const int nq = masked_words(max_seqlen_q), nk = masked_words(max_seqlen_k);
  const int64_t items = num_seqs * nq * nk;
  if (items == 0) return WCN_SUCCESS;
  hipStream_t s = (hipStream_t)stream;
  uint32_t *qw = (uint32_t*)q_words, *kw = (uint32_t*)k_words;
  switch (src_dtype) {
    case WCN_F32:
      mask_pack_launch<float>(src, src_rows, src_pitch, q_cols, threshold, key_index, cu_q, cu_k, items, nq, nk, qw, q_pitch, kw,
                              k_pitch, s);
      break;
    case WCN_F16:
      mask_pack_launch<_Float16>(src, src_rows, src_pitch, q_cols, threshold, key_index, cu_q, cu_k, items, nq, nk, qw, q_pitch, kw,
                                 k_pitch, s);
      break;
    case WCN_BF16:
      mask_pack_launch<__bf16>(src, src_rows, src_pitch, q_cols, threshold, key_index, cu_q, cu_k, items, nq, nk, qw, q_pitch, kw,
                               k_pitch, s);
      break;
    default:
      mask_pack_launch<uint8_t>(src, src_rows, src_pitch, q_cols, threshold, key_index, cu_q, cu_k, items, nq, nk, qw, q_pitch, kw,
                                k_pitch, s);
  }
  if (release_full_rows)
    hipLaunchKernelGGL(attn_mask_release_kernel, dim3(masked_grid(num_seqs * nq)), dim3(256), 0, s, cu_q, cu_k, num_seqs * nq, nq,
                       qw, q_pitch, kw, k_pitch);
  return hipGetLastError() == hipSuccess ? WCN_SUCCESS : WCN_ERROR_KERNEL_EXECUTION;
}

int wcn_attn_varlen_kv_fwd_m(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                             const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs, int64_t total_q, int64_t total_k,
                             int32_t heads, int32_t head_dim, int32_t max_seqlen_q, int32_t max_seqlen_k, float softmax_scale,
                             int32_t dtype, void* out, float* lse, const int32_t* q_words, int64_t q_pitch, const int32_t* k_words,
                             int64_t k_pitch, int32_t k_splits, void* workspace, size_t workspace_bytes, wcn_stream_t stream) {
  if (k_splits < 0) return WCN_ERROR_INVALID_PARAMETERS;
  const int st = attn_kv_check(q, q_stride, k, v, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, head_dim,
                               max_seqlen_q, max_seqlen_k, softmax_scale, wcn_attn_varlen_supported(head_dim, dtype));
  if (st != WCN_SUCCESS) return st;
  if (total_q > 0 && (!out || !lse || !aligned_to(out, 16))) return WCN_ERROR_INVALID_PARAMETERS;
  if (!masked_words_ok(q_words, q_pitch, k_words, k_pitch, total_q, total_k, max_seqlen_q, max_seqlen_k))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (k_splits == 0) k_splits = wcn_attn_varlen_k_splits(num_seqs, max_seqlen_q, max_seqlen_k, heads, 0);
  const size_t need = wcn_attn_varlen_ksplit_workspace_bytes(total_q, total_k, heads, head_dim, 1, k_splits, 0);
  if (need > 0 && (!workspace || workspace_bytes < need || !aligned_to(workspace, 16))) return WCN_ERROR_INVALID_PARAMETERS;
  if (num_seqs == 0 || total_q == 0 || max_seqlen_q == 0) return WCN_SUCCESS;
  const AttnCall c{q, k, v, q_stride, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, max_seqlen_q, max_seqlen_k,
                   softmax_scale};
  const AttnMaskWords mk{(const uint32_t*)q_words, (const uint32_t*)k_words, q_pitch, k_pitch};
  // the workspace of wcn_attn_varlen_kv_fwd_s: o [k_splits, total_q, heads, head_dim], then ml [k_splits, total_q, heads, 2]
  float* o = (float*)workspace;
  const AttnKSplit ks{k_splits, total_q, o, o + (size_t)k_splits * (size_t)total_q * (size_t)heads * (size_t)head_dim};
  return masked_dispatch(head_dim, dtype, [&](auto t, auto d) {
    return masked_fwd_t<decltype(t), decltype(d)::value>(c, mk, out, lse, ks, (hipStream_t)stream);
  });
}

int wcn_attn_varlen_kv_bwd_m(const void* dout, const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride,
                             const void* out, const float* lse, const int32_t* cu_q, const int32_t* cu_k, int64_t num_seqs,
                             int64_t total_q, int64_t total_k, int32_t heads, int32_t head_dim, int32_t max_seqlen_q,
                             int32_t max_seqlen_k, float softmax_scale, int32_t dtype, void* dq, int64_t dq_stride, void* dk,
                             void* dv, int64_t dkv_stride, const int32_t* q_words, int64_t q_pitch, const int32_t* k_words,
                             int64_t k_pitch, int32_t k_splits, void* workspace, size_t workspace_bytes, wcn_stream_t stream) {
  if (k_splits < 0) return WCN_ERROR_INVALID_PARAMETERS;
  const int st = attn_kv_check(q, q_stride, k, v, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, head_dim,
                               max_seqlen_q, max_seqlen_k, softmax_scale, wcn_attn_varlen_supported(head_dim, dtype));
  if (st != WCN_SUCCESS) return st;
  const int64_t hd = (int64_t)heads * head_dim;
  if (dq_stride < hd || dkv_stride < hd || (dq_stride & 7) || (dkv_stride & 7)) return WCN_ERROR_INVALID_PARAMETERS;
  if (total_q > 0 && (!dout || !out || !lse || !dq)) return WCN_ERROR_INVALID_PARAMETERS;
  if (total_k > 0 && (!dk || !dv)) return WCN_ERROR_INVALID_PARAMETERS;
  if (!aligned_to(dout, 16) || !aligned_to(out, 16) || !aligned_to(dq, 16) || !aligned_to(dk, 16) || !aligned_to(dv, 16) ||
      !aligned_to(workspace, 16))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (!masked_words_ok(q_words, q_pitch, k_words, k_pitch, total_q, total_k, max_seqlen_q, max_seqlen_k))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (k_splits == 0) k_splits = wcn_attn_varlen_k_splits(num_seqs, max_seqlen_q, max_seqlen_k, heads, 1);
  const size_t need = wcn_attn_varlen_ksplit_workspace_bytes(total_q, total_k, heads, head_dim, 1, k_splits, 1);
  if (workspace_bytes < need || (need > 0 && !workspace)) return WCN_ERROR_INVALID_PARAMETERS;
  if (num_seqs == 0 || (total_q == 0 && total_k == 0)) return WCN_SUCCESS;
  // the workspace of wcn_attn_varlen_kv_bwd_s at q_splits = 1: the dQ partials [k_splits, total_q, heads, head_dim] (none at
  // k_splits = 1), then delta [total_q, heads]
  const size_t delta_bytes = (size_t)total_q * (size_t)heads * sizeof(float);
  float* delta = (float*)((char*)workspace + (need - delta_bytes));
  const AttnKSplit ks{k_splits, total_q, (float*)workspace, nullptr};
  const AttnCall c{q, k, v, q_stride, kv_stride, cu_q, cu_k, num_seqs, total_q, total_k, heads, max_seqlen_q, max_seqlen_k,
                   softmax_scale};
  const AttnMaskWords mk{(const uint32_t*)q_words, (const uint32_t*)k_words, q_pitch, k_pitch};
  return masked_dispatch(head_dim, dtype, [&](auto t, auto d) {
    return masked_bwd_t<decltype(t), decltype(d)::value>(c, mk, dout, out, lse, dq, dq_stride, dk, dv, dkv_stride, delta, ks,
                                                         (hipStream_t)stream);
  });
}
